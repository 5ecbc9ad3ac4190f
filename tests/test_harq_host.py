"""CPU: the interface of HARQ retransmissions with soft combining -- the C ABI
additions (header, exports, ctypes signatures, argument checks that return
before the device is touched), the code-block split against the model in
tests/harq_model.py, and the Python keywords.  The kernels are checked on the
GPU in tests/test_gpu_harq.py."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import harq_model as M

NEW_SYMBOLS = ['lte_plan_create_harq', 'lte_plan_harq_set_round', 'lte_plan_harq_tx_used', 'lte_plan_harq_info',
               'lte_harq_code_block_bits']
TB_SIZES = [435, 6121, 12217, 27760]


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def test_header_declares_the_new_names():
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % name, text, re.M), name
    assert re.search(r'^typedef struct \{ int32_t max_tx; int32_t rv_seq\[8\]; int64_t G; \} lte_harq_desc;$',
                     text, re.M)
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)


def test_library_exports_them_with_signatures(C):
    import ctypes
    lib = C.load()
    for name in NEW_SYMBOLS:
        assert name in C._SIGS, name
        assert getattr(lib, name).argtypes == C._SIGS[name][1], name
    assert lib.lte_version() == 3 and C.ABI_VERSION == 3
    assert [f[0] for f in C.HarqDesc._fields_] == ['max_tx', 'rv_seq', 'G']
    assert ctypes.sizeof(C.HarqDesc) == 48      # 9 int32, 4 bytes of padding, int64


def test_plan_entries_refuse_a_null_plan(C):
    import ctypes
    lib = C.load()
    d, hd, h = C.PlanDesc(), C.HarqDesc(), ctypes.c_void_p()
    assert lib.lte_plan_create_harq(None, ctypes.byref(hd), ctypes.byref(h)) == C.LTE_EINVAL
    assert lib.lte_plan_create_harq(ctypes.byref(d), None, ctypes.byref(h)) == C.LTE_EINVAL
    assert lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), None) == C.LTE_EINVAL
    assert lib.lte_plan_harq_set_round(None, 0) == C.LTE_EINVAL
    out = np.zeros(4, dtype=np.uint8)
    assert lib.lte_plan_harq_tx_used(None, C.ptr(out, C.U8), 4) == C.LTE_EINVAL
    info = np.zeros(8, dtype=np.int64)
    assert lib.lte_plan_harq_info(None, C.ptr(info, C.c_i64), 8) == C.LTE_EINVAL


def test_create_harq_refuses_other_chains_without_a_device(C):
    """Every chain but LTE_CHAIN_CODED is LTE_EUNSUP (SFBC-coded included), and
    bad HARQ settings LTE_EINVAL, from the first checks of the shared body."""
    import ctypes
    lib = C.load()
    hd, h = C.HarqDesc(), ctypes.c_void_p()
    hd.max_tx = 4
    for chain in (C.CHAIN_UNCODED, C.CHAIN_SIMO, C.CHAIN_SFBC, C.CHAIN_SFBC_CODED, C.CHAIN_SPATIAL,
                  C.CHAIN_BEAMFORMING):
        d = C.PlanDesc()
        d.chain = chain
        assert lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)) == C.LTE_EUNSUP, chain
        assert b'HARQ' in lib.lte_last_error()
    d = C.PlanDesc()
    d.chain = C.CHAIN_CODED
    for max_tx, rv0, G in ((0, 0, 0), (9, 0, 0), (2, 4, 0), (2, -1, 0), (2, 0, -6)):
        hd.max_tx, hd.rv_seq[0], hd.G = max_tx, rv0, G
        assert lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)) == C.LTE_EINVAL
        assert b'HARQ' in lib.lte_last_error()


def _cb_bits(C, n_bits, bps, G, n_max=16):
    K, E = np.zeros(max(n_max, 1), dtype=np.int32), np.zeros(max(n_max, 1), dtype=np.int32)
    c = C.load().lte_harq_code_block_bits(n_bits, bps, G, C.ptr(K, C.I32), C.ptr(E, C.I32), n_max)
    return c, K[:max(c, 0)].tolist(), E[:max(c, 0)].tolist()


def _budgets(O, n_bits, bps):
    """G = 0, a multiple of bps whose G / bps is not a multiple of C (gamma != 0
    where C > 1), and the largest budget sum(3K + 18)."""
    Ks = [p[0] for p in O.segmentation_plan(n_bits + 24)]
    C_ = len(Ks)
    full = sum(3 * K + 18 for K in Ks)
    Gp = int(0.45 * full) // bps
    while C_ > 1 and Gp % C_ == 0:
        Gp += 1
    return Ks, [0, Gp * bps, full]


@pytest.mark.parametrize('bps', [2, 4, 6])
@pytest.mark.parametrize('n_bits', TB_SIZES)
def test_code_block_bits_equal_the_models_split(C, oracle, n_bits, bps):
    """G = sum(3K + 18) is a budget the rule itself accepts only where it is a
    multiple of bps (3K + 18 = 2 mod 4: not at 16-QAM with an odd block count)
    and the blocks are of one size (with two sizes the even split gives the
    smaller block more than its 3K + 18); elsewhere the model and the library
    both refuse it."""
    Ks, budgets = _budgets(oracle, n_bits, bps)
    for G in budgets:
        try:
            mK, mE = M.split(oracle, n_bits, bps, G)
        except ValueError:
            assert G == budgets[2] and (len(set(Ks)) > 1 or G % bps)
            assert _cb_bits(C, n_bits, bps, G)[0] == C.LTE_EINVAL, (n_bits, bps, G)
            continue
        c, K, E = _cb_bits(C, n_bits, bps, G)
        assert (c, K, E) == (len(Ks), mK, mE), (n_bits, bps, G)
        assert sum(E) == (G or sum(3 * k + 12 for k in Ks))
        if G and len(Ks) > 1 and G != budgets[2]:
            assert (G // bps) % len(Ks) != 0 and len(set(E)) == 2, (G, E)


@pytest.mark.parametrize('bps', [2, 4, 6])
@pytest.mark.parametrize('n_bits', TB_SIZES)
def test_code_block_bits_refuse_bad_budgets(C, oracle, n_bits, bps):
    Ks = [p[0] for p in oracle.segmentation_plan(n_bits + 24)]
    n, full = len(Ks), sum(3 * K + 18 for K in Ks)
    lib = C.load()
    for G in (bps * n * 100 + 1, (full // bps + n) * bps, bps * (n - 1), -bps):
        if G == 0:
            continue           # one code block: bps * (n - 1) is the G = 0 default, not a refusal
        assert _cb_bits(C, n_bits, bps, G)[0] == C.LTE_EINVAL, (n_bits, bps, G)
        assert b'HARQ' in lib.lte_last_error()
        with pytest.raises(ValueError):
            M.split(oracle, n_bits, bps, G)
    if n > 1:
        assert _cb_bits(C, n_bits, bps, 0, n_max=n - 1)[0] == C.LTE_EINVAL
        assert b'n_max' in lib.lte_last_error()
    assert _cb_bits(C, n_bits, bps, 0, n_max=0)[0] == C.LTE_EINVAL
    assert _cb_bits(C, n_bits, 3, 0)[0] == C.LTE_EINVAL


def test_model_split_is_36212_on_a_hand_case(oracle):
    """TB 12217: K = 4096, 4096, 4160.  G = 17000 at 16-QAM: G' = 4250, gamma = 2,
    so block 0 takes 4 * 1416 and blocks 1, 2 take 4 * 1417."""
    assert M.split(oracle, 12217, 4, 17000) == ([4096, 4096, 4160], [5664, 5668, 5668])
    assert M.seed_t(5, 0) == 5 and M.seed_t(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C14


def test_run_harq_grid_signature():
    import lte_phy
    sig = inspect.signature(lte_phy.OFDMSimulator.run_harq_grid)
    got = [(p.name, p.default) for p in sig.parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD][1:]
    assert got == [('snr_range', inspect.Parameter.empty), ('num_trials', inspect.Parameter.empty), ('seed', 0),
                   ('n_bits', None), ('coded_bits', None), ('max_tx', 4), ('rv_seq', (0, 2, 3, 1)),
                   ('frames_per_call', 4096), ('rank', 0), ('world_size', 1), ('turbo_iters', 8)]
    grid = list(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters)
    assert grid == ['self', 'snr_range', 'num_trials', 'seed', 'coded', 'num_rx', 'n_bits', 'frames_per_call', 'rank',
                    'world_size', 'turbo_iters', 'mimo', 'velocity_kmh', 'frequency_ghz', 'spatial', 'beamforming',
                    'early_stop']


def test_plan_keyword():
    from lte_phy import engine
    p = inspect.signature(engine.Plan.__init__).parameters['harq']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert callable(engine.Plan.run_harq) and callable(engine.Plan.harq_round)


def test_run_harq_grid_refuses_bad_requests_without_a_device():
    """Raised from the argument checks and the host-only split, before any plan
    (or device) is needed."""
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    for kw in (dict(coded=False), dict(num_rx=2), dict(mimo='sfbc'), dict(mimo='spatial'), dict(mimo='beamforming')):
        with pytest.raises(ValueError, match='coded SISO'):
            sim.run_harq_grid([0.0], 1, n_bits=435, **kw)
    for kw in (dict(max_tx=0), dict(max_tx=9), dict(max_tx=4, rv_seq=(0, 2)), dict(rv_seq=(0, 2, 3, 4))):
        with pytest.raises(ValueError, match='max_tx'):
            sim.run_harq_grid([0.0], 1, n_bits=435, **kw)
    for G in (641, 2 * (3 * 464 + 18) + 2, -2):
        with pytest.raises(ValueError, match='HARQ'):
            sim.run_harq_grid([0.0], 1, n_bits=435, coded_bits=G)
    with pytest.raises(ValueError):
        sim.run_harq_grid([0.0], 0, n_bits=435)


def test_channel_coding_all_is_unchanged():
    from lte_phy import channel_coding
    assert len(channel_coding.__all__) == 18
