"""Shape tables of the normalisation / reduction kernel tests, shared by tests/test_norm_dispatch_cpu.py (every reachable launch
plan is hit by a case) and tests/test_gpu_norm_reduce.py (every case against a float64 reference).

The launch plans come from the library's own host-side queries (include/sg2im_hip.h: sg_instnorm_plan, sg_batchnorm_plan,
sg_channel_sum_plan) -- the functions the launches themselves are planned with -- so a table entry names a kernel form by
shape alone and cannot drift from the dispatch.
"""
import contextlib
import ctypes

from scene_generation_amd._hip import CONST

# include/sg2im_hip.h: SG_IN_*
IN_THREE_PASS_WAVE, IN_THREE_PASS_BLOCK, IN_REG, IN_VEC, IN_BIG = (
    CONST['SG_IN_' + n] for n in ('THREE_PASS_WAVE', 'THREE_PASS_BLOCK', 'REG', 'VEC', 'BIG'))
IN_KIND_NAMES = {IN_THREE_PASS_WAVE: 'three_pass_wave', IN_THREE_PASS_BLOCK: 'three_pass_block', IN_REG: 'reg', IN_VEC: 'vec',
                 IN_BIG: 'big'}
INSTNORM_REG_VALUES = (0, 1, 2)          # the option instnorm_reg: three-pass kernels only / + register-resident / + float4 forms

# ---- InstanceNorm: (N, C, H, W, mean offset).  Every case runs under each instnorm_reg, 16-byte aligned and through a 4-byte
# storage offset.  HW = 1, 2, 3; a non-multiple-of-4 plane in every G range; the benchmark planes 8x8 at 1024 channels,
# 128 x 128 and 256 x 256 (big kernels); N C mostly not a multiple of the planes per workgroup (16 at G = 16, 4 at G = 64).
# Mean offset 100 (std ~1) in at least one case of every kernel family: a single-pass variance would cancel there.
INSTNORM_CASES = [
    (3, 5, 1, 1, 0.0),          # HW 1: z = 0 exactly
    (2, 7, 1, 2, 0.0),
    (3, 3, 1, 3, 0.0),
    (1, 3, 2, 2, 0.0),          # vec <16, 1> with 3 of 64 planes live
    (3, 7, 5, 6, 0.0),          # reg <16, 2>
    (3, 5, 7, 9, 100.0),        # reg <16, 4>, three-pass wave
    (2, 1024, 8, 8, 0.0),       # benchmark: vec <16, 1>
    (3, 5, 10, 10, 0.0),        # vec <64, 1>, reg <64, 2>
    (2, 3, 15, 17, 0.0),        # reg <64, 4>
    (2, 5, 16, 16, 0.0),
    (2, 3, 17, 17, 0.0),        # reg <64, 8>
    (2, 5, 22, 22, 0.0),        # vec <64, 2>
    (2, 3, 31, 31, 0.0),        # reg <64, 16>
    (3, 3, 32, 32, 100.0),      # vec <64, 4>
    (2, 3, 37, 37, 0.0),        # reg <256, 8>, three-pass block
    (2, 1, 40, 40, 100.0),      # vec <256, 2>
    (2, 3, 63, 63, 0.0),        # reg <256, 16>
    (1, 3, 64, 64, 0.0),        # vec <256, 4>
    (1, 3, 85, 85, 0.0),        # reg <256, 32>
    (1, 3, 80, 80, 0.0),        # vec <256, 8>
    (1, 3, 99, 99, 0.0),        # reg <256, 64> / bwd reg <1024, 16>
    (2, 3, 128, 128, 0.0),      # benchmark: vec <256, 16> / bwd vec <1024, 4>
    (1, 3, 129, 129, 0.0),      # reg <1024, 32> / bwd three-pass block
    (1, 2, 100, 200, 0.0),      # vec <1024, 8> / bwd big
    (1, 3, 256, 256, 100.0),    # benchmark: big
    (1, 2, 191, 191, 0.0),      # three-pass block (odd plane beyond the register forms)
]

# ---- BatchNorm: (shape, bn_blocks option or None).  Flat and per-plane apply, S = 1 and S > 1 statistics slices, the two-pass
# statistics branch (slices > BN_REG * 256 = 10240 elements: more than 512 * 10240 elements per channel, with few slices), an
# empty trailing slice (S - 1 slices of ceil(cnt / S) already cover cnt), BatchNorm1d.
BATCHNORM_CASES = [
    ((6, 5, 4, 4), None),               # flat apply, S = 1
    ((37, 8), None),                    # BatchNorm1d (HW = 1)
    ((64, 3, 9, 9), None),              # flat apply, S = 5
    ((2, 3, 16, 16), None),             # per-plane apply, S = 1
    ((4, 3, 32, 32), None),             # per-plane apply, S = 4
    ((8, 16, 31, 31), None),            # per-plane apply, S = 7
    ((3, 1, 1, 375467), 1100),          # empty trailing slice: 1099 slices of 1025 cover the 1126401 elements
    ((2, 1, 1700, 1700), 256),          # two-pass statistics: 256 slices of 22579 elements
]

# ---- channel_sum: (N, C, HW, with workspace).  S = 1; S > 1 with HW >= 256 and HW < 256 (both loops of
# channel_sum_partial_kernel); the C >= 256, cnt <= 16384 override (against C = 255, which splits); the no-workspace fallback;
# the 64-slice cap.
CHANNEL_SUM_CASES = [
    (2, 8, 100, True),                  # S = 1 (cnt < 8192)
    (4, 16, 4096, True),                # S = 4, HW >= 256
    (512, 8, 100, True),                # S = 12, HW < 256
    (4, 255, 4096, True),               # S = 4
    (4, 256, 4096, True),               # the same reduction length at 256 channels: the single-stage override
    (4, 16, 4096, False),               # no workspace: single stage
    (64, 2, 16384, True),               # S = 64 (cap)
    (3, 5, 7919, True),                 # S = 5, odd plane
]


def channel_sum_ws_bytes(lib, C):
    return lib.sg_channel_sum_ws_bytes(C)


def _ints(n):
    return [ctypes.c_int(0) for _ in range(n)]


def _ptr(v):
    return ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)


def instnorm_plan(lib, bwd, HW, aligned16):
    """-> (kind, G, E) of sg_instnorm_plan under the current option instnorm_reg"""
    k, g, e = _ints(3)
    rc = lib.sg_instnorm_plan(int(bwd), int(HW), int(aligned16), _ptr(k), _ptr(g), _ptr(e))
    assert rc == 0
    return k.value, g.value, e.value


def batchnorm_plan(lib, N, C, HW):
    """-> (S, apply_form, stats_two_pass) of sg_batchnorm_plan under the current option bn_blocks"""
    s, a, t = _ints(3)
    assert lib.sg_batchnorm_plan(int(N), int(C), int(HW), _ptr(s), _ptr(a), _ptr(t)) == 0
    return s.value, a.value, t.value


def channel_sum_plan(lib, N, C, HW, ws_bytes):
    """-> S of sg_channel_sum_plan (1: the single-stage kernel)"""
    s = ctypes.c_int(0)
    assert lib.sg_channel_sum_plan(int(N), int(C), int(HW), int(ws_bytes), _ptr(s)) == 0
    return s.value


def bn_hw(shape):
    n = 1
    for d in shape[2:]:
        n *= d
    return n


def bn_empty_trailing_slice(N, HW, S):
    cnt = N * HW
    chunk = -(-cnt // S)
    return (S - 1) * chunk >= cnt


@contextlib.contextmanager
def option(name, value):
    """set a library option for the block and restore it afterwards (value None: leave it alone)"""
    from scene_generation_amd import _hip
    if value is None:
        yield
        return
    saved = _hip.get_option(name)
    _hip.set_option(name, value)
    try:
        yield
    finally:
        _hip.set_option(name, saved)


def instnorm_kernel_name(bwd, kind, G, E):
    """the kernel's name as tools/isa_report.py shortens it"""
    d = 'bwd' if bwd else 'fwd'
    if kind == IN_VEC:
        return 'instnorm_%s_vec_kernel<%d, %d>' % (d, G, E)
    if kind == IN_REG:
        return 'instnorm_%s_reg_kernel<%d, %d>' % (d, G, E)
    if kind == IN_BIG:
        return 'instnorm_%s_big_kernel' % d
    return 'instnorm_%s_kernel<%s>' % (d, 'true' if kind == IN_THREE_PASS_WAVE else 'false')
