"""ctypes binding of libsg2im_hip.so.

Everything is parsed from include/sg2im_hip.h (the single source of truth for the C ABI), once, at import, so nothing on the Python
side can drift from the header:
  PROTOS   the prototypes: {name: (restype, [argtypes], [argnames])}
  STRUCTS  every ``typedef struct NAME { ... } NAME;`` as a ctypes.Structure subclass (also a module attribute: _hip.sgConvDesc, ...)
  CONST    every enumerator of every ``enum { ... };`` and every ``#define SG_NAME <integer>``: {name: int}
A new struct or constant of the header needs no Python declaration.  The parser is strict: a field type, a declarator, an
enumerator or a define it does not understand raises at import.  There is NO fallback either way: if the shared library is missing
or a symbol cannot be resolved, import of the compute path fails loudly.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'sg2im_hip.h')
LIB_PATH = os.environ.get('SG_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libsg2im_hip.so')   # SG_LIB_PATH: kernel-variant builds

_STRUCT_RE = r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;'
_ENUM_RE = r'enum\s*(\w*)\s*\{(.*?)\}\s*;'
_INT = r'-?\s*(?:0[xX][0-9a-fA-F]+|\d+)'
_FIELD_TYPES = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'double': ctypes.c_double,
                'int': ctypes.c_int, 'size_t': ctypes.c_size_t}


def _strip_comments(src):
    return re.sub(r'//[^\n]*', ' ', re.sub(r'/\*.*?\*/', ' ', src, flags=re.S))


def parse_types(src):
    """header text -> (structs, const): {name: ctypes.Structure subclass} with the header's field order, and {name: int} of the
    enumerators and the integer ``#define SG_*``.  Raises ValueError, naming the struct / enum / define, for anything but
    ``<int32_t|int64_t|float|double|int|size_t> name[, name[n]...];`` fields, ``NAME = <integer>`` enumerators and integer defines."""
    src = _strip_comments(src)
    structs, const = {}, {}

    def define(name, value, where):
        value = int(value.replace(' ', ''), 0)
        if const.setdefault(name, value) != value:
            raise ValueError('%s: %s = %d, but it is %d earlier in the header' % (where, name, value, const[name]))

    for m in re.finditer(_STRUCT_RE, src, flags=re.S):
        name, fields = m.group(1), []
        if m.group(3) != name or name in structs:
            raise ValueError('struct %s: typedef name %s differs from the tag, or the struct is declared twice' % (name, m.group(3)))
        for line in filter(None, (ln.strip() for ln in m.group(2).split(';'))):
            ty, decls = (line.split(None, 1) + [''])[:2]
            if ty not in _FIELD_TYPES:
                raise ValueError('struct %s: unknown field type in "%s;"' % (name, line))
            for decl in decls.split(','):
                f = re.fullmatch(r'\s*([A-Za-z_]\w*)\s*(?:\[\s*(\d+)\s*\])?\s*', decl)
                if f is None:
                    raise ValueError('struct %s: cannot parse "%s" in "%s;"' % (name, decl.strip(), line))
                fields.append((f.group(1), _FIELD_TYPES[ty] * int(f.group(2)) if f.group(2) else _FIELD_TYPES[ty]))
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields})
    rest = re.sub(_STRUCT_RE, ' ', src, flags=re.S)
    if re.search(r'\bstruct\b', rest):
        raise ValueError('a struct the parser does not understand: "%s"' % rest[re.search(r'\bstruct\b', rest).start():][:60])
    for m in re.finditer(_ENUM_RE, rest, flags=re.S):
        items = [it.strip() for it in m.group(2).split(',') if it.strip()]
        where = 'enum %s{ %s ... }' % (m.group(1) + ' ' if m.group(1) else '', items[0].split('=')[0].strip() if items else '')
        for it in items:
            e = re.fullmatch(r'([A-Za-z_]\w*)\s*=\s*(%s)' % _INT, it)
            if e is None:
                raise ValueError('%s: enumerator "%s" is not NAME = <integer> (implicit values are not supported)' % (where, it))
            define(e.group(1), e.group(2), where)
    if re.search(r'\benum\b', re.sub(_ENUM_RE, ' ', rest, flags=re.S)):
        raise ValueError('an enum the parser does not understand (expected "enum { ... };")')
    for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(SG_\w+)(.*)$', src, flags=re.M):
        v = re.fullmatch(r'\s+(?:\(\s*(%s)\s*\)|(%s))\s*' % (_INT, _INT), m.group(2))
        if v is None:
            raise ValueError('#define %s: "%s" is not an integer literal' % (m.group(1), m.group(2).strip()))
        define(m.group(1), v.group(1) or v.group(2), '#define %s' % m.group(1))
    return structs, const


STRUCTS, CONST = parse_types(open(HEADER).read())
globals().update(STRUCTS)           # _hip.sgConvDesc, _hip.sgRectDesc, _hip.sgWgradPlan, ...


def plan_dict(s):
    """the fields of a struct instance as a dict: arrays as tuples, a field named ``reserved`` dropped"""
    out = {}
    for n, _ in s._fields_:
        if n != 'reserved':
            v = getattr(s, n)
            out[n] = tuple(v) if isinstance(v, ctypes.Array) else v
    return out


_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
            'size_t': ctypes.c_size_t, 'double': ctypes.c_double, 'sgStream': ctypes.c_void_p}


def _ctype(decl):
    decl = decl.strip()
    if decl == 'void':
        return None
    if '*' in decl:
        if 'char' in decl:
            return ctypes.c_char_p
        if decl.replace('const', '').strip().startswith('double'):
            return ctypes.POINTER(ctypes.c_double)
        if re.match(r'(const\s+)?int64_t\s*\*\s*(launches)?$', decl) and 'launches' in decl:
            return ctypes.POINTER(ctypes.c_int64)
        return ctypes.c_void_p
    words = decl.replace('const', '').split()
    if words[:2] == ['long', 'long']:
        return ctypes.c_longlong
    return _SCALARS[words[0]]


def parse_header(path=HEADER):
    """-> {name: (restype, [argtypes], [argnames])} for every function the header declares."""
    src = _strip_comments(open(path).read())
    src = re.sub(_STRUCT_RE, ' ', src, flags=re.S)
    src = re.sub(_ENUM_RE, ' ', src, flags=re.S)
    protos = {}
    for m in re.finditer(r'([A-Za-z_][\w\s\*]*?)\b(sg_\w+)\s*\(([^)]*)\)\s*;', src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if 'char' in ret:
            restype = ctypes.c_char_p
        elif ret == 'size_t':
            restype = ctypes.c_size_t
        else:
            restype = ctypes.c_int
        argtypes, argnames = [], []
        if args and args != 'void':
            for a in args.split(','):
                a = a.strip()
                nm = re.search(r'(\w+)\s*$', a).group(1)
                ty = a[:a.rfind(nm)].strip()
                if nm == 'launches':
                    argtypes.append(ctypes.POINTER(ctypes.c_int64))
                else:
                    argtypes.append(_ctype(ty))
                argnames.append(nm)
        protos[name] = (restype, argtypes, argnames)
    return protos


PROTOS = parse_header()
_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def lib():
    """Load (once) and return the shared library with typed prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HipLibraryMissing(
            '%s not found: the MI355X compute path has no fallback. Build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` or scene_generation_amd/csrc/build.sh' % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes, _) in PROTOS.items():
        fn = getattr(L, name)           # AttributeError if the .so does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = L
    if os.environ.get('SG_LEGACY_ALIGN_CORNERS', '0') == '1':
        L.sg_set_legacy_align_corners(1)
    return L


def last_error():
    return lib().sg_last_error_string().decode()


def check(rc, name):
    if rc != 0:
        raise RuntimeError('%s failed (rc=%d): %s' % (name, rc, last_error()))


# ---- tuning / debugging switches of the library (include/sg2im_hip.h: sg_set_option) --------------------------------
OPTION_GENERATION = 0


def set_option(name, value):
    """Change a launch-plan switch of the library at run time (they are otherwise fixed when the library is loaded: compiled-in
    default, or the environment variable SG_<NAME>)."""
    check(lib().sg_set_option(name.encode(), int(value)), 'sg_set_option')
    global OPTION_GENERATION
    OPTION_GENERATION += 1          # shape-only queries memoised on the conv descs (ops/_core._q) may depend on an option


_opt_cache = {}


def option_cached(name):
    """current value of a switch, re-read from the library only after a set_option (per-launch callers)"""
    hit = _opt_cache.get(name)
    if hit is None or hit[0] != OPTION_GENERATION:
        hit = _opt_cache[name] = (OPTION_GENERATION, get_option(name))
    return hit[1]


def get_option(name):
    v = ctypes.c_int(0)
    check(lib().sg_get_option(name.encode(), ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)), 'sg_get_option')
    return v.value


def options():
    """{name: (current value, compiled-in default)} of every switch"""
    L = lib()
    out = {}
    for i in range(L.sg_num_options()):
        name = L.sg_option_name(i).decode()
        out[name] = (get_option(name), L.sg_option_default(i))
    return out
