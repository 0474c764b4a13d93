"""The launch plans of the InstanceNorm, BatchNorm and channel-sum dispatch (host-side queries of libsg2im_hip.so, no GPU): the
shape tables of tests/norm_cases.py -- what tests/test_gpu_norm_reduce.py runs against float64 -- reach every plan the
dispatch can choose, and every kernel those plans name exists in the built code object."""
import functools
import os
import re
import shutil

import pytest

import norm_cases as NC
from scene_generation_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW_MAX = 70000


@functools.lru_cache(maxsize=None)
def _reachable_instnorm_plans(lib):
    """{(reg, bwd, kind, G, E)} over HW = 1..HW_MAX, both alignments, every instnorm_reg"""
    plans = set()
    for reg in NC.INSTNORM_REG_VALUES:
        with NC.option('instnorm_reg', reg):
            for bwd in (0, 1):
                for aligned in (1, 0):
                    for hw in range(1, HW_MAX + 1):
                        plans.add((reg, bwd) + NC.instnorm_plan(lib, bwd, hw, aligned))
    return plans


def _case_instnorm_plans(lib):
    plans = set()
    for reg in NC.INSTNORM_REG_VALUES:
        with NC.option('instnorm_reg', reg):
            for (n, c, h, w, _) in NC.INSTNORM_CASES:
                for bwd in (0, 1):
                    for aligned in (1, 0):
                        plans.add((reg, bwd) + NC.instnorm_plan(lib, bwd, h * w, aligned))
    return plans


def test_plan_kinds_match_the_header():
    text = open(os.path.join(ROOT, 'include', 'sg2im_hip.h')).read()
    m = re.search(r'enum\s*\{\s*(SG_IN_THREE_PASS_WAVE[^}]*)\}', text)
    assert m, 'SG_IN_* enum not found in the header'
    vals = dict((k, int(v)) for k, v in re.findall(r'(SG_IN_\w+)\s*=\s*(\d+)', m.group(1)))
    assert vals == {'SG_IN_THREE_PASS_WAVE': NC.IN_THREE_PASS_WAVE, 'SG_IN_THREE_PASS_BLOCK': NC.IN_THREE_PASS_BLOCK,
                    'SG_IN_REG': NC.IN_REG, 'SG_IN_VEC': NC.IN_VEC, 'SG_IN_BIG': NC.IN_BIG}


def test_instnorm_cases_cover_every_reachable_plan(capsys):
    lib = _hip.lib()
    reachable = _reachable_instnorm_plans(lib)
    covered = _case_instnorm_plans(lib)
    assert covered <= reachable
    missing = sorted(reachable - covered)
    assert not missing, 'InstanceNorm plans no norm_cases entry reaches: %s' % missing
    kinds = set(p[2] for p in reachable)
    assert kinds == {NC.IN_THREE_PASS_WAVE, NC.IN_THREE_PASS_BLOCK, NC.IN_REG, NC.IN_VEC, NC.IN_BIG}
    with capsys.disabled():
        print('\nnorm_cases covers all %d reachable InstanceNorm plans (%d distinct kernels)'
              % (len(reachable), len(set((p[1],) + p[2:] for p in reachable))))


def test_instnorm_plan_follows_the_option_and_alignment():
    lib = _hip.lib()
    with NC.option('instnorm_reg', 2):
        assert NC.instnorm_plan(lib, 0, 16384, 1) == (NC.IN_VEC, 256, 16)         # 128 x 128, the benchmark plane
        assert NC.instnorm_plan(lib, 1, 16384, 1) == (NC.IN_VEC, 1024, 4)
        assert NC.instnorm_plan(lib, 0, 16384, 0) == (NC.IN_REG, 256, 64)         # unaligned: no float4 form
        assert NC.instnorm_plan(lib, 1, 16384, 0) == (NC.IN_REG, 1024, 16)
        assert NC.instnorm_plan(lib, 0, 65536, 1) == (NC.IN_BIG, 1024, 0)
        assert NC.instnorm_plan(lib, 0, 65536, 0)[0] == NC.IN_THREE_PASS_BLOCK
        assert NC.instnorm_plan(lib, 0, 64, 1) == (NC.IN_VEC, 16, 1)
        assert NC.instnorm_plan(lib, 0, 63, 1) == (NC.IN_REG, 16, 4)
    with NC.option('instnorm_reg', 1):
        assert NC.instnorm_plan(lib, 0, 16384, 1) == (NC.IN_REG, 256, 64)
        assert NC.instnorm_plan(lib, 1, 65536, 1) == (NC.IN_BIG, 1024, 0)
    with NC.option('instnorm_reg', 0):
        assert NC.instnorm_plan(lib, 0, 1024, 1)[0] == NC.IN_THREE_PASS_WAVE
        assert NC.instnorm_plan(lib, 1, 1025, 1)[0] == NC.IN_THREE_PASS_BLOCK
        assert NC.instnorm_plan(lib, 0, 65536, 1)[0] == NC.IN_THREE_PASS_BLOCK
    assert _hip.get_option('instnorm_reg') == _hip.options()['instnorm_reg'][1]


def _bn_class(S, apply_form, two_pass):
    return (apply_form, S > 1, two_pass)


def test_batchnorm_cases_cover_every_reachable_plan():
    lib = _hip.lib()
    reachable = set()
    for N in (1, 2, 3, 8, 64, 1056):
        for C in (1, 3, 16, 64, 128, 512):
            for HW in (1, 16, 81, 255, 256, 961, 4096, 16384):
                reachable.add(_bn_class(*NC.batchnorm_plan(lib, N, C, HW)))
    with NC.option('bn_blocks', 256):
        reachable.add(_bn_class(*NC.batchnorm_plan(lib, 2, 1, 1700 * 1700)))
    covered, empty_tail = set(), False
    for shape, blocks in NC.BATCHNORM_CASES:
        N, C, HW = shape[0], shape[1], NC.bn_hw(shape)
        with NC.option('bn_blocks', blocks):
            S, a, t = NC.batchnorm_plan(lib, N, C, HW)
        covered.add(_bn_class(S, a, t))
        empty_tail |= S > 1 and NC.bn_empty_trailing_slice(N, HW, S)
    assert reachable <= covered, sorted(reachable - covered)
    assert (1, True, 1) in covered and (0, True, 0) in covered and (1, False, 0) in covered and (0, False, 0) in covered
    assert empty_tail, 'no BatchNorm case has an empty trailing statistics slice'
    assert any(len(shape) == 2 for shape, _ in NC.BATCHNORM_CASES)                # BatchNorm1d
    with NC.option('bn_blocks', 256):
        assert NC.batchnorm_plan(lib, 2, 1, 1700 * 1700) == (256, 1, 1)
    assert NC.batchnorm_plan(lib, 2, 1, 1700 * 1700)[2] == 0                         # 4096 slices: register-resident


def test_channel_sum_cases_cover_every_reachable_plan():
    lib = _hip.lib()
    cls = lambda S, HW: (S > 1, S > 1 and HW >= 256)
    reachable = set()
    for N in (1, 2, 4, 16, 64, 512):
        for C in (1, 3, 16, 255, 256, 1024):
            for HW in (1, 16, 100, 255, 256, 4096, 16384):
                for ws in (True, False):
                    wsb = NC.channel_sum_ws_bytes(lib, C) if ws else 0
                    reachable.add(cls(NC.channel_sum_plan(lib, N, C, HW, wsb), HW))
    covered = set()
    S_of = {}
    for (N, C, HW, ws) in NC.CHANNEL_SUM_CASES:
        S = NC.channel_sum_plan(lib, N, C, HW, NC.channel_sum_ws_bytes(lib, C) if ws else 0)
        covered.add(cls(S, HW))
        S_of[(N, C, HW, ws)] = S
    assert reachable <= covered, sorted(reachable - covered)
    assert S_of[(4, 255, 4096, True)] > 1 and S_of[(4, 256, 4096, True)] == 1       # the C >= 256 override
    assert S_of[(4, 16, 4096, True)] > 1 and S_of[(4, 16, 4096, False)] == 1        # no workspace
    assert S_of[(64, 2, 16384, True)] == 64
    assert NC.channel_sum_plan(lib, 4, 16, 4096, 4 * 16 * 4 - 1) == 1               # workspace one byte short


def test_reachable_kernels_exist_in_the_code_object():
    from tools import isa_report
    if not (os.path.isfile(isa_report.DEFAULT_LIB) and shutil.which('objcopy')
            and os.path.isfile(os.path.join(isa_report.LLVM, 'clang-offload-bundler'))):
        pytest.skip('needs the built library and the ROCm LLVM tools')
    names = set(k['name'] for k in isa_report.kernels())
    want = set(NC.instnorm_kernel_name(p[1], *p[2:]) for p in _reachable_instnorm_plans(_hip.lib()))
    want |= {'bn_stats_kernel', 'bn_final_kernel', 'bn_apply_kernel', 'bn_apply_flat_kernel', 'bn_bwd_stats_kernel',
             'bn_bwd_final_kernel', 'bn_bwd_apply_kernel', 'bn_bwd_apply_flat_kernel', 'channel_sum_kernel',
             'channel_sum_partial_kernel', 'channel_sum_final_kernel'}
    missing = sorted(want - names)
    assert not missing, missing
