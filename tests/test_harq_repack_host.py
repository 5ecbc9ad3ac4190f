"""CPU: the interface of re-packing the unacknowledged frames of a HARQ process --
the C ABI additions (header, exports, ctypes signatures, refusals that return
before the device is touched), the rule lte_harq_repack_rule against its
restatement in tests/harq_repack_model.py, and the Python keywords.  The
kernels are checked on the GPU in tests/test_gpu_harq_repack.py (the C refusal
of a plan without HARQ too: a plan needs the device)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import harq_repack_model as RM

NEW_SYMBOLS = ['lte_plan_set_harq_repack', 'lte_plan_harq_repack', 'lte_plan_harq_repack_info',
               'lte_harq_repack_rule']


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % name, text, re.M), name
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)       # additions only
    assert re.search(r'^typedef struct \{ int32_t max_tx; int32_t rv_seq\[8\]; int64_t G; \} lte_harq_desc;$',
                     text, re.M)


def test_library_exports_them_with_signatures(C):
    lib = C.load()
    for name in NEW_SYMBOLS:
        assert name in C._SIGS, name
        assert getattr(lib, name).argtypes == C._SIGS[name][1], name
    assert lib.lte_version() == 3 and C.ABI_VERSION == 3


def test_entries_refuse_null_arguments(C):
    lib = C.load()
    assert lib.lte_plan_set_harq_repack(None, 1) == C.LTE_EINVAL
    assert lib.lte_plan_set_harq_repack(None, 0) == C.LTE_EINVAL
    assert lib.lte_plan_harq_repack(None) == C.LTE_EINVAL
    info = np.zeros(7, dtype=np.int64)
    assert lib.lte_plan_harq_repack_info(None, C.ptr(info, C.c_i64), 7) == C.LTE_EINVAL
    acked, out = np.zeros(4, dtype=np.uint8), np.zeros(6, dtype=np.int64)
    assert lib.lte_harq_repack_rule(None, 4, 1, C.ptr(out, C.c_i64)) == C.LTE_EINVAL
    assert lib.lte_harq_repack_rule(C.ptr(acked, C.U8), 4, 1, None) == C.LTE_EINVAL
    assert lib.lte_harq_repack_rule(C.ptr(acked, C.U8), 0, 1, C.ptr(out, C.c_i64)) == C.LTE_EINVAL
    assert lib.lte_harq_repack_rule(C.ptr(acked, C.U8), 4, 0, C.ptr(out, C.c_i64)) == C.LTE_EINVAL


def test_a_plan_without_harq_refuses_the_keyword_before_the_device():
    from lte_phy import engine
    with pytest.raises(ValueError, match='harq='):
        engine.Plan(N=128, Nc=76, cp_len=9, bps=2, n_sym=0, chain=1, channel=0, n_bits=435, harq_repack=True)


def group(valid, active, rs):
    """Acknowledgements of one group of `valid` lanes with `active` unacknowledged, in a random lane order."""
    a = np.ones(valid, dtype=np.uint8)
    a[rs.permutation(valid)[:active]] = 0
    return a


def masks():
    """Named hand cases, then random ones: B a multiple of 64 or not, groups of
    every class, few or many active lanes."""
    rs = np.random.RandomState(20)
    full, fin = lambda v=64: group(v, v, rs), lambda v=64: group(v, 0, rs)
    mix = lambda a, v=64: group(v, a, rs)
    hand = {
        'all finished': (np.concatenate([fin(), fin(), fin(7)]), 2),
        'all active': (np.concatenate([full(), full(), full(7)]), 2),
        'one mixed group, never packed': (np.concatenate([fin(), mix(1), full()]), 4),
        'one mixed partial group': (np.concatenate([fin(), full(), mix(3, 7)]), 4),
        'P == M': (np.concatenate([mix(50), mix(50), fin()]), 4),
        'P > cap': (np.concatenate([fin(), mix(40), mix(40), mix(40)]), 1),
        'P < M, P <= cap': (np.concatenate([fin(), mix(40), mix(40), mix(40), full()]), 2),
        'partly filled, partial last group': (np.concatenate([fin(), mix(20), mix(24), full(), mix(4, 7)]), 2),
        'one frame': (np.zeros(1, dtype=np.uint8), 1),
        'one frame acknowledged': (np.ones(1, dtype=np.uint8), 1),
    }
    out = [(k, a, cap) for k, (a, cap) in hand.items()]
    for i in range(300):
        B = int(rs.choice([rs.randint(1, 64), 64 * rs.randint(1, 12), rs.randint(65, 900)]))
        G = -(-B // 64)
        acked = np.concatenate([group(min(64, B - 64 * g), 0, rs) for g in range(G)])
        for g in range(G):
            valid = min(64, B - 64 * g)
            kind = rs.randint(4)
            active = 0 if kind == 0 else valid if kind == 1 else rs.randint(0, valid + 1) if kind == 2 else \
                rs.randint(0, min(valid, 6) + 1)
            acked[64 * g:64 * g + valid] = group(valid, active, rs)
        cap = int(rs.choice([1, RM.pack_cap(G), RM.pack_cap(G) + 1]))
        out.append(('random %d' % i, acked, cap))
    return out


def test_the_rule_equals_its_restatement(C):
    seen = {'pack': 0, 'P == M': 0, 'over cap': 0, 'M == 1': 0, 'partial': 0}
    for tag, acked, cap in masks():
        got, want = C.harq_repack_rule(acked, cap), RM.rule(acked, cap)
        assert got == want, (tag, got, want)
        # 0 / 255 and 0 / 1 are the same acknowledgements
        assert C.harq_repack_rule(acked * 255, cap) == want, tag
        seen['pack'] += want['pack']
        seen['P == M'] += want['M'] >= 1 and want['P'] == want['M']
        seen['over cap'] += want['M'] >= 1 and want['P'] < want['M'] and want['P'] > cap
        seen['M == 1'] += want['M'] == 1
        seen['partial'] += len(acked) % 64 != 0
        if want['M'] == 1:
            assert not want['pack'], tag
        if want['pack']:
            assert want['waves_on'] < want['waves_off'], tag
        else:
            assert want['waves_on'] == want['waves_off'], tag
    assert all(v >= 3 for v in seen.values()), seen


def test_the_hand_cases_say_what_they_are_named_for(C):
    hand = {tag: C.harq_repack_rule(a, cap) for tag, a, cap in masks()[:10]}
    z = dict(M=0, A=0, P=0, pack=False)
    assert hand['all finished'] == dict(z, waves_off=0, waves_on=0)
    assert hand['all active'] == dict(z, waves_off=3, waves_on=3)
    assert hand['one mixed group, never packed'] == dict(M=1, A=1, P=1, pack=False, waves_off=2, waves_on=2)
    assert hand['one mixed partial group'] == dict(M=1, A=3, P=1, pack=False, waves_off=2, waves_on=2)
    assert hand['P == M'] == dict(M=2, A=100, P=2, pack=False, waves_off=2, waves_on=2)
    assert hand['P > cap'] == dict(M=3, A=120, P=2, pack=False, waves_off=3, waves_on=3)
    assert hand['P < M, P <= cap'] == dict(M=3, A=120, P=2, pack=True, waves_off=4, waves_on=3)
    assert hand['partly filled, partial last group'] == dict(M=3, A=48, P=1, pack=True, waves_off=4, waves_on=2)


def test_keywords_are_keyword_only_and_off_by_default():
    import lte_phy
    from lte_phy import engine
    p = inspect.signature(engine.Plan.__init__).parameters['harq_repack']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert callable(engine.Plan.set_harq_repack) and callable(engine.Plan.harq_repack_info)
    sig = inspect.signature(lte_phy.OFDMSimulator.run_harq_grid)
    p = sig.parameters['repack']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    # the positional signature is as it was
    got = [q.name for q in sig.parameters.values() if q.kind is q.POSITIONAL_OR_KEYWORD]
    assert got == ['self', 'snr_range', 'num_trials', 'seed', 'n_bits', 'coded_bits', 'max_tx', 'rv_seq',
                   'frames_per_call', 'rank', 'world_size', 'turbo_iters']
    assert 'repack' not in inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters
    assert len(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters) == 17


def test_plan_key_tells_the_setting_apart():
    from lte_phy import engine
    kw = dict(N=128, Nc=76, cp_len=9, bps=2, n_sym=0, chain=1, channel=0, n_bits=435,
              harq=dict(max_tx=4, rv_seq=(0, 2, 3, 1), coded_bits=0))
    plain, off, on = (engine.plan_key(**dict(kw), **x)[0] for x in ({}, {'harq_repack': False}, {'harq_repack': True}))
    assert plain == off and on != off


def test_run_harq_grid_still_refuses_other_chains_with_the_keyword():
    import lte_phy
    s = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    with pytest.raises(ValueError, match='coded SISO'):
        s.run_harq_grid([0.0], 1, n_bits=435, num_rx=2, repack=True)
