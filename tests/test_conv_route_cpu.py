"""The kernel route of a conv (ops.conv_route) on the host: the four special-kernel predicates of the library are disjoint -- the
invariant that lets conv_route ask them in any order -- and the route follows the desc, the second source / sparse list and the
three switches, never a stale memo.  No GPU: the library loads without one and every ``*_supported`` query is host-only."""
import ctypes
import itertools

import pytest

from scene_generation_amd import _hip, ops
from scene_generation_amd._hip import sgConvDesc
from scene_generation_amd.ops import _core

PREDICATES = ('sg_conv2d_wino24_supported', 'sg_conv2d_head_supported', 'sg_conv2d_wino_supported', 'sg_conv2d_smallm_supported')


def test_special_route_predicates_are_disjoint():
    L = _hip.lib()
    fns = [getattr(L, n) for n in PREDICATES]
    claimed = [0] * len(fns)
    swept = 0
    for N, C1, H, Cout, KS, stride, pad, reflect, ups in itertools.product(
            (1, 2, 4, 32), (3, 16, 64, 128, 192, 256, 512), (4, 7, 8, 16, 31, 32, 64, 128), (1, 3, 4, 64, 128, 256, 512),
            (1, 3, 4, 7), (1, 2), range(4), (0, 1), (1, 2)):
        OH = _core.conv_out_size(H, KS, stride, pad, ups)
        if (reflect and pad == 0) or pad >= H * ups or OH <= 0:
            continue
        d = sgConvDesc(N, C1, 0, H, H, Cout, KS, stride, pad, reflect, ups, OH, OH, 0, 0)
        ans = [bool(f(ctypes.byref(d))) for f in fns]
        assert sum(ans) <= 1, ('more than one special kernel claims', [getattr(d, f) for f, _ in d._fields_], ans)
        claimed = [c + a for c, a in zip(claimed, ans)]
        swept += 1
    assert swept > 100000
    # the descs of tests/head_smallm_cases.py (rows, probes, both sides of every inequality of the head and small-M predicates), and
    # what the square sweep above does not reach: non-square planes, planes at the head's LDS budget, channel counts around its floor
    import head_smallm_cases as HS
    extra = [HS.desc_of(f) for f in HS.CASES + HS.PROBES + [e[1] for e in HS.HEAD_EDGES + HS.SMALLM_EDGES]]
    for (H, W), C1, Cout, KS, pad, reflect in itertools.product(
            ((4, 4), (5, 8), (8, 5), (17, 68), (17, 132), (2, 256), (2, 257), (40, 38), (49, 49), (49, 50), (50, 50)), (1, 2, 5, 15, 16, 17, 40, 128),
            (1, 2, 3, 4, 5, 128), (1, 3, 4, 7), range(5), (0, 1)):
        OH, OW = _core.conv_out_size(H, KS, 1, pad), _core.conv_out_size(W, KS, 1, pad)
        if (reflect and pad == 0) or pad >= min(H, W) or OH <= 0 or OW <= 0:
            continue
        extra.append(sgConvDesc(2, C1, 0, H, W, Cout, KS, 1, pad, reflect, 1, OH, OW, 0, 0))
    assert len(extra) > 10000
    before = list(claimed)
    for d in extra:
        ans = [bool(f(ctypes.byref(d))) for f in fns]
        assert sum(ans) <= 1, ('more than one special kernel claims', [getattr(d, f) for f, _ in d._fields_], ans)
        claimed = [c + a for c, a in zip(claimed, ans)]
    head, smallm = PREDICATES.index('sg_conv2d_head_supported'), PREDICATES.index('sg_conv2d_smallm_supported')
    assert claimed[head] > before[head] + 100 and claimed[smallm] > before[smallm] + 100
    assert all(c > 0 for c in claimed), dict(zip(PREDICATES, claimed))     # (a sweep that reaches no desc of a class proves nothing)


def _desc(N, C1, H, Cout, KS, pad, reflect, C2=0):
    OH = _core.conv_out_size(H, KS, 1, pad)
    return _core._conv_desc(N, C1, C2, H, H, Cout, KS, 1, pad, reflect, 1, OH, OH, 0, 0)


# one desc per class (the shapes of tests/test_gpu_conv_routes.py): route with every switch on, the switch that owns it
CLASSES = [
    ('generic', dict(N=1, C1=3, H=4, Cout=8, KS=3, pad=1, reflect=False), 'ROUTE_GENERIC', None),
    ('head', dict(N=1, C1=16, H=4, Cout=1, KS=1, pad=0, reflect=False), 'ROUTE_HEAD', 'HEADCONV'),
    ('smallm', dict(N=1, C1=3, H=4, Cout=3, KS=7, pad=3, reflect=True), 'ROUTE_SMALLM', None),
    ('wino', dict(N=2, C1=128, H=16, Cout=128, KS=3, pad=1, reflect=True), 'ROUTE_WINO', 'WINOGRAD'),
    ('wino24', dict(N=1, C1=128, H=31, Cout=128, KS=4, pad=2, reflect=False), 'ROUTE_WINO24', 'WINOGRAD24'),
]
SWITCHES = ('WINOGRAD', 'WINOGRAD24', 'HEADCONV')


@pytest.fixture
def switches_on():
    saved = {k: getattr(_core, k) for k in SWITCHES}
    for k in SWITCHES:
        setattr(ops, k, True)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def test_route_constants_are_six_distinct_values():
    assert len({ops.ROUTE_GENERIC, ops.ROUTE_SPARSE, ops.ROUTE_WINO, ops.ROUTE_WINO24, ops.ROUTE_HEAD, ops.ROUTE_SMALLM}) == 6


@pytest.mark.parametrize('name,shape,route,switch', CLASSES, ids=[c[0] for c in CLASSES])
def test_conv_route_of_each_class(switches_on, name, shape, route, switch):
    d = _desc(**shape)
    assert ops.conv_route(d, False, False) == getattr(ops, route)
    assert ops.conv_route(d, False, False) == getattr(ops, route)          # (answered from the memo)
    # a second source or a sparse list: never a special kernel
    assert ops.conv_route(d, True, False) == ops.ROUTE_GENERIC
    assert ops.conv_route(d, False, True) == ops.ROUTE_SPARSE
    assert ops.conv_route(d, True, True) == ops.ROUTE_SPARSE
    # each switch off sends its own class, and only that one, to the generic route -- on the same desc object, memo or not
    for k in SWITCHES:
        setattr(ops, k, False)
        try:
            assert ops.conv_route(d, False, False) == (ops.ROUTE_GENERIC if k == switch else getattr(ops, route)), k
        finally:
            setattr(ops, k, True)
        assert ops.conv_route(d, False, False) == getattr(ops, route)


def test_conv_route_honours_a_library_option_changed_between_two_calls(switches_on):
    """the library's ``wino24`` option switches its F(2x2,4x4) predicate off: the route of the SAME desc object follows it"""
    d = _desc(**CLASSES[4][1])
    saved = _hip.get_option('wino24')
    assert saved and ops.conv_route(d, False, False) == ops.ROUTE_WINO24
    _hip.set_option('wino24', 0)
    try:
        assert ops.conv_route(d, False, False) == ops.ROUTE_GENERIC
    finally:
        _hip.set_option('wino24', saved)
    assert ops.conv_route(d, False, False) == ops.ROUTE_WINO24
