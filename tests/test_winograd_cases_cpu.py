"""The Winograd test material of tests/winograd_cases.py, checked on the host: the float64 restatements of the three forms equal the
direct convolution, the pairs are adjoint, the float32 restatement meets its own hard bound and gives a usable rms baseline, mutants
of it are caught, and -- through the library's host-only query sg_conv2d_wino_plan -- the case table reaches every value of every
plan field and every case's expected plan holds under each of its option sets."""
import ctypes
import os
import re

import numpy as np
import pytest

import winograd_cases as WC
from gpu_harness import options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = lambda c: c['name']


@pytest.fixture(scope='module')
def lib():
    from scene_generation_amd import _hip
    return _hip.lib()


def option_sets(case):
    """the case's own options, and each toggle of OPTION_TOGGLES that names the case on top of them"""
    return [dict(case['opts'])] + [dict(case['opts'], **o) for (n, o, _) in WC.OPTION_TOGGLES if n == case['name']]


# =============================================================================================
# the references
# =============================================================================================
@pytest.mark.parametrize('case', WC.CASES, ids=IDS)
def test_float64_restatement_equals_the_direct_convolution(case):
    r = WC.case_refs(case)
    got = WC.restate(case, r['form'], r['inp'], np.float64)
    for k in ('y', 'gx', 'gw'):
        scale = float(np.abs(r['ref'][k]).max())
        assert got[k].shape == r['ref'][k].shape
        assert float(np.abs(got[k] - r['ref'][k]).max()) <= 1e-12 * scale, (case['name'], k)


@pytest.mark.parametrize('name', WC.PROBE_CASES)
def test_forward_and_gradients_are_adjoint_in_float64(name):
    """<y(x, w), gy> = <x, gx(gy, w)> = <w, gw(gy, x)> for the restated forms (y is bilinear in x and w)"""
    case = WC.BY_NAME[name]
    r = WC.case_refs(case)
    got = WC.restate(case, r['form'], r['inp'], np.float64)
    x, w, gy = [np.asarray(r['inp'][k], dtype=np.float64) for k in ('x', 'w', 'gy')]
    a, b, c = float((got['y'] * gy).sum()), float((x * got['gx']).sum()), float((w * got['gw']).sum())
    scale = float((np.abs(got['y']) * np.abs(gy)).sum())
    assert abs(a - b) <= 1e-12 * scale and abs(a - c) <= 1e-12 * scale, (a, b, c)


@pytest.mark.parametrize('case', WC.CASES, ids=IDS)
def test_float32_restatement_meets_the_hard_bound_and_gives_a_baseline(case):
    r = WC.case_refs(case)
    for k in ('y', 'gx', 'gw'):
        base = r[k + '_rms32']
        assert np.isfinite(base) and base > 0.0, (case['name'], k, base)
        assert (r[k + '_bound'] > 0).all()
        ratio, _ = WC.check(r[k + '_r32'], r['ref'][k], r[k + '_bound'], base, '%s %s' % (case['name'], k), rms_line=False)
        assert ratio < 0.05, 'the float32 restatement uses %.3f of the hard bound' % ratio


def test_chunked_sums_stay_within_the_rms_line():
    """the chunked channel sum of the kernels (256 + 128, 256 + 256) is a different order of the same terms: it has to sit under the
    sequential baseline's factor, or the line could not be asked of the kernels"""
    for name, key, kw in (('f43_16_384to128_8x8', 'y', dict(fwd_chunk=256)), ('f43_16_512to128_8x8', 'y', dict(fwd_chunk=256)),
                          ('f43_16_128to384_8x8', 'gx', dict(dgrad_chunk=256)), ('f24_8_128to256_20x14_p1', 'gw', dict(wgrad_chunk=288))):
        case = WC.BY_NAME[name]
        r = WC.case_refs(case)
        got = WC.restate(case, r['form'], r['inp'], np.float32, which=(key,), **kw)[key]
        WC.check(got, r['ref'][key], r[key + '_bound'], r[key + '_rms32'], name + ' chunked ' + key)


MUTANTS = WC.mutants()
# what the issue lists, by the names above
MUTANT_KINDS = {
    'one transform coefficient off by one': ('f43_output_coefficient_off_by_one', 'f23_input_coefficient_off_by_one', 'f24_filter_coefficient_off_by_one'),
    'reflection replaced by clamp': ('reflection_replaced_by_clamp', 'reflection_replaced_by_clamp_f23'),
    "one tile's column offset shifted": ('last_tile_column_shifted',),
    'the last chunk of a chunked sum dropped': ('last_chunk_of_forward_sum_dropped', 'last_chunk_of_dgrad_sum_dropped', 'last_k_chunk_of_f24_wgrad_dropped'),
    'a 2x2 upsample sum-back that misses one pixel': ('upsample_sum_back_misses_one_pixel',),
    'the F24 clipped edge tile written unclipped': ('f24_clipped_edge_tile_written_unclipped',),
}


def test_mutant_list_covers_the_kinds():
    names = {m[0] for m in MUTANTS}
    assert set().union(*MUTANT_KINDS.values()) == names


@pytest.mark.parametrize('mutant', MUTANTS, ids=lambda m: m[0])
def test_mutant_of_the_float32_restatement_fails_a_criterion(mutant):
    mname, cname, kw, outs = mutant
    case = WC.BY_NAME[cname]
    r = WC.case_refs(case)
    kw = dict(kw)
    form = kw.pop('form', r['form'])
    got = WC.restate(case, form, r['inp'], np.float32, which=outs, **kw)
    # the unmutated restatement with the same chunking passes: the mutation alone makes the difference
    clean = WC.restate(case, r['form'], r['inp'], np.float32, which=outs, **{k: v for k, v in kw.items() if k != 'mutant'})
    for k in outs:
        assert not WC.fails(clean[k], r['ref'][k], r[k + '_bound'], r[k + '_rms32']), (mname, k)
        assert WC.fails(got[k], r['ref'][k], r[k + '_bound'], r[k + '_rms32']), '%s is not caught on %s of %s' % (mname, k, cname)


# =============================================================================================
# the plans, through the library's host query
# =============================================================================================
def test_plan_struct_and_constants_match_the_header():
    text = open(os.path.join(ROOT, 'include', 'sg2im_hip.h')).read()
    body = re.search(r'typedef struct sgWinoPlan \{(.*?)\} sgWinoPlan;', text, re.S).group(1)
    names = [n.strip() for decl in re.findall(r'int32_t ([^;]*);', body) for n in decl.split(',')]
    assert tuple(names) == WC.PLAN_FIELDS
    enums = dict((k, int(v)) for k, v in re.findall(r'\b(SG_W\w+) = (\d+)', text))
    for k, v in (('SG_WINO_FWD', WC.WINO_FWD), ('SG_WINO_DGRAD', WC.WINO_DGRAD), ('SG_WINO_WGRAD', WC.WINO_WGRAD),
                 ('SG_WINO_FWD_INSTNORM', WC.WINO_FWD_INSTNORM), ('SG_WINO_DGRAD_INSTNORM', WC.WINO_DGRAD_INSTNORM),
                 ('SG_WINO24_FWD', WC.WINO24_FWD), ('SG_WINO24_DGRAD', WC.WINO24_DGRAD), ('SG_WINO24_WGRAD', WC.WINO24_WGRAD),
                 ('SG_WA_X', WC.WA_X), ('SG_WA_W', WC.WA_W), ('SG_WA_Y', WC.WA_Y), ('SG_WA_GY', WC.WA_GY), ('SG_WA_GX', WC.WA_GX),
                 ('SG_WA_GW', WC.WA_GW), ('SG_WA_ALL', WC.WA_ALL), ('SG_WS_UT', WC.WS_UT), ('SG_WS_V', WC.WS_V), ('SG_WS_YTP', WC.WS_YTP),
                 ('SG_WF_UNSUPPORTED', WC.WF_UNSUPPORTED), ('SG_WF_F23_GENERIC', WC.WF_F23_GENERIC), ('SG_WF_F23_ADJOINT', WC.WF_F23_ADJOINT),
                 ('SG_WF_F43', WC.WF_F43), ('SG_WF_F24', WC.WF_F24), ('SG_WK_NONE', WC.WK_NONE), ('SG_WK_IN_LDS', WC.WK_IN_LDS),
                 ('SG_WK_IN_GENERAL', WC.WK_IN_GENERAL), ('SG_WK_WT_LDS', WC.WK_WT_LDS), ('SG_WK_WT_PLAIN', WC.WK_WT_PLAIN),
                 ('SG_WK_FOLD_CELLS', WC.WK_FOLD_CELLS), ('SG_WK_FOLD_WALK', WC.WK_FOLD_WALK), ('SG_WK_FOLD_F43', WC.WK_FOLD_F43),
                 ('SG_WK_FOLD_PAD_UPSAMPLE', WC.WK_FOLD_PAD_UPSAMPLE), ('SG_WSRC_SAVED', WC.WSRC_SAVED), ('SG_WSRC_REBUILT', WC.WSRC_REBUILT)):
        assert enums[k] == v, k


def test_option_defaults_are_the_librarys(lib):
    from scene_generation_amd import _hip
    names = [lib.sg_option_name(i).decode() for i in range(lib.sg_num_options())]
    for k, v in WC.OPTION_DEFAULTS.items():
        assert lib.sg_option_default(names.index(k)) == v, k
        assert _hip.get_option(k) == v, '%s is not at its default' % k


def _plans_of(lib, case, opts):
    """[(entry, saved mask, plan)] of the case under the options, every saved-operand combination the entry accepts"""
    d = WC.case_desc(case)
    out = []
    with options(opts):
        for entry in WC.case_entries(case):
            for sm in WC.saved_masks(case, entry, opts):
                out.append((entry, sm, WC.wino_plan(lib, d, entry, WC.case_align(case, entry), sm)))
        if case['name'] in WC.FUSED_CASES and opts.get('wino_in_fuse', 1) and opts.get('wino_reuse', 1):
            for entry in (WC.WINO_FWD_INSTNORM, WC.WINO_DGRAD_INSTNORM):
                for sm in WC.saved_masks(case, entry, opts):
                    out.append((entry, sm, WC.wino_plan(lib, d, entry, WC.WA_ALL, sm)))
    return out


@pytest.mark.parametrize('case', WC.CASES, ids=IDS)
def test_expected_plan_holds_under_every_option_set(lib, case):
    for opts in option_sets(case):
        for entry, sm, got in _plans_of(lib, case, opts):
            what = (case['name'], opts, WC.ENTRY_NAMES[entry], sm)
            assert got is not None, (what, lib.sg_last_error_string().decode())
            exp = WC.expected_plan(case, entry, opts, saved=sm)
            assert got == exp, (what, {k: (got[k], exp[k]) for k in got if got[k] != exp[k]})
            if entry == WC.WINO_DGRAD and sm == 0:
                assert got['form'] == case['dgrad_form'], what
            if opts == case['opts'] and sm == 0:
                for k, v in case['claims'].get(WC.ENTRY_NAMES[entry], {}).items():
                    assert got[k] == v, (what, k, got[k], v)
    with options(case['opts']):
        d = WC.case_desc(case)
        if case['family'] == 'F24':
            assert lib.sg_conv2d_wino24_supported(ctypes.byref(d)) == 1 and lib.sg_conv2d_wino_supported(ctypes.byref(d)) == 0
        else:
            assert lib.sg_conv2d_wino_supported(ctypes.byref(d)) == 1 and lib.sg_conv2d_wino24_supported(ctypes.byref(d)) == 0


@pytest.mark.parametrize('toggle', WC.OPTION_TOGGLES, ids=lambda t: '%s-%s' % (t[0], '_'.join('%s%d' % kv for kv in t[1].items())))
def test_option_toggle_shows_in_the_plan(lib, toggle):
    name, opts, claims = toggle
    case = WC.BY_NAME[name]
    names = {v: k for k, v in enumerate(WC.ENTRY_NAMES)}
    d = WC.case_desc(case)
    with options(dict(case['opts'], **opts)):
        for ename, fields in claims.items():
            got = WC.wino_plan(lib, d, names[ename], WC.case_align(case, names[ename]), 0)
            assert got is not None, (name, opts, ename, lib.sg_last_error_string().decode())
            for k, v in fields.items():
                assert got[k] == v, (name, opts, ename, k, got[k], v)
    # each toggle leaves its default
    for k, v in opts.items():
        assert WC.OPTION_DEFAULTS[k] != v, (k, v)


def test_every_listed_option_value_is_toggled():
    want = {('wino_wt', 0), ('wino_fold_cells', 0), ('wino_reuse', 0), ('wino_in_fuse', 0), ('wino_pipe', 1), ('wino_gemm_tile', 1),
            ('wino_gemm_tile', 2), ('w43_kfold', 0), ('w43_kfold', 128), ('w43_nsub', 2), ('w43_wgrad_tile', 1), ('w43_wgrad_tile', 2),
            ('w24_small', 0), ('w24_s', 1), ('w24_s', 3), ('w24_gemm_tile', 0), ('w24_gemm_tile', 1)}
    have = {kv for (_, o, _) in WC.OPTION_TOGGLES for kv in o.items()}
    assert want <= have, want - have
    # (the defaults -- wino_pipe 2, wino_gemm_tile 0, w43_kfold 256, w43_nsub 1, w43_wgrad_tile 0, w24_gemm_tile 2 -- are every case's plain run)


def test_table_reaches_every_value_of_every_plan_field(lib):
    seen = set()
    for case in WC.CASES:
        for opts in option_sets(case):
            for entry, sm, got in _plans_of(lib, case, opts):
                assert got is not None, (case['name'], opts, entry, sm)
                seen |= WC.plan_values(got)
    assert WC.ALL_PLAN_VALUES <= seen, sorted(WC.ALL_PLAN_VALUES - seen)


@pytest.mark.parametrize('case', [c for c in WC.CASES if c['family'] != 'F24'], ids=IDS)
def test_saved_operand_sizes_agree_with_the_plan(lib, case):
    d = WC.case_desc(case)
    with options(case['opts']):
        ut, v, ytp = [getattr(lib, 'sg_conv2d_wino_%s_floats' % n)(ctypes.byref(d)) for n in ('ut', 'v', 'ytp')]
        fwd = WC.wino_plan(lib, d, WC.WINO_FWD)
        xi = 36 if fwd['form'] == WC.WF_F43 else 16
        for size, entry, bit, per in ((ut, WC.WINO_FWD, WC.WS_UT, None), (v, WC.WINO_FWD, WC.WS_V, d.C1), (ytp, WC.WINO_DGRAD, WC.WS_YTP, d.Cout)):
            accepted = WC.wino_plan(lib, d, entry, WC.WA_ALL, bit)
            assert (size > 0) == (accepted is not None), (case['name'], entry, bit, size)
            if size:
                assert size == (xi * d.C1 * d.Cout if per is None else xi * accepted['P'] * per), (case['name'], bit, size)
        both = WC.wino_plan(lib, d, WC.WINO_WGRAD, WC.WA_ALL, WC.WS_V | WC.WS_YTP)
        assert (both is not None) == (v > 0 and ytp > 0)
        if both is not None:
            assert both['wgrad_src'] == WC.WSRC_SAVED and both['in_kernel'] == WC.WK_NONE


def test_plan_query_rejects_what_the_entry_points_reject(lib):
    P = WC.sgWinoPlan()
    q = lambda d, e, a=WC.WA_ALL, s=0, p=P: lib.sg_conv2d_wino_plan(ctypes.byref(d), e, a, s, ctypes.byref(p) if p is not None else None)
    f43 = WC.case_desc(WC.BY_NAME['f43_16_128to128_8x8'])
    assert q(f43, WC.WINO_FWD) == 0
    assert q(f43, -1) != 0 and q(f43, 8) != 0 and q(f43, WC.WINO_FWD, p=None) != 0
    assert q(f43, WC.WINO_FWD, 64) != 0 and q(f43, WC.WINO_FWD, WC.WA_ALL, 8) != 0
    # F(4x4,3x3): an unaligned operand is an error, never another form
    for entry, bits in ((WC.WINO_FWD, (WC.WA_X, WC.WA_W, WC.WA_Y)), (WC.WINO_DGRAD, (WC.WA_GY, WC.WA_GX, WC.WA_W)), (WC.WINO_WGRAD, (WC.WA_X, WC.WA_GY)),
                        (WC.WINO_FWD_INSTNORM, (WC.WA_X, WC.WA_W, WC.WA_Y)), (WC.WINO_DGRAD_INSTNORM, (WC.WA_GY, WC.WA_GX, WC.WA_W))):
        for b in bits:
            assert q(f43, entry, WC.WA_ALL & ~b) != 0, (entry, b)
        assert 'aligned' in lib.sg_last_error_string().decode()
    # saved operands on descs that cannot use them
    z = WC.case_desc(WC.BY_NAME['f23z_2_128to128_16x16'])
    assert q(z, WC.WINO_FWD, s=WC.WS_V) != 0 and q(z, WC.WINO_FWD, s=WC.WS_UT) != 0 and q(z, WC.WINO_DGRAD, s=WC.WS_YTP) != 0
    assert q(z, WC.WINO_WGRAD, s=WC.WS_V | WC.WS_YTP) != 0
    assert q(z, WC.WINO_FWD_INSTNORM) != 0                     # no fused form outside F(4x4,3x3)
    a = WC.case_desc(WC.BY_NAME['f23a_8_128to128_8x8'])
    assert q(a, WC.WINO_DGRAD, WC.WA_ALL & ~WC.WA_GY, WC.WS_YTP) != 0         # unaligned gy: generic form, which keeps no Ytp
    assert q(a, WC.WINO_FWD, WC.WA_ALL & ~WC.WA_W, WC.WS_UT) != 0              # the transposed twin needs the LDS weight kernel
    with WC.option('wino_in_fuse', 0):
        assert q(f43, WC.WINO_FWD_INSTNORM) != 0
    # unsupported descs: 192 channels, a tile count that is no multiple of 128, F(2x2,4x4) under w24_pmin tiles
    for d, entry in ((WC.make_desc(8, 192, 8, 8, 192, 3, 1, 1, True, 1, 8, 8), WC.WINO_FWD),
                     (WC.make_desc(4, 128, 8, 8, 128, 3, 1, 1, True, 1, 8, 8), WC.WINO_FWD),
                     (WC.make_desc(2, 128, 12, 12, 128, 4, 1, 1, False, 1, 11, 11), WC.WINO24_FWD),
                     (f43, WC.WINO24_FWD), (WC.case_desc(WC.BY_NAME['f24_4_128to128_17x17_p2']), WC.WINO_FWD)):
        assert q(d, entry) != 0
        assert 'unsupported desc' in lib.sg_last_error_string().decode()
    d192 = WC.make_desc(8, 192, 8, 8, 192, 3, 1, 1, True, 1, 8, 8)
    assert lib.sg_conv2d_wino_supported(ctypes.byref(d192)) == 0               # (mask_net's 192 channels run the direct kernel)
