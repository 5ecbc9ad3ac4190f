"""CPU: the interface of the coded TM4 chain (LTE_CHAIN_SPATIAL_CODED: spatial
multiplexing with the soft MMSE / ZF / MRC detector and turbo coding) -- the
header line, the ctypes constant, the checks lte_plan_create makes before the
device is touched, the Python entry points' signatures, and the model of
tests/spatial_coded_model.py on its own: every ladder case of
tests/test_gpu_spatial_coded.py straddles the turbo cliff, so an agreement
there says something; the model stays finite where the rule clamps; and r_cpu,
the unit of the GPU tests' bars, is measured here.  The kernels are checked on
the GPU in tests/test_gpu_spatial_coded.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import spatial_coded_model as M


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def test_header_and_binding_name_the_chain(C):
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    assert re.search(r'^\s*LTE_CHAIN_SPATIAL_CODED = 8$', text, re.M)
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)      # an additive value: no new version
    assert C.CHAIN_SPATIAL_CODED == 8 and C.load().lte_version() == 3
    from lte_phy import engine
    assert engine.chain_is_coded(C.CHAIN_SPATIAL_CODED) and engine.chain_is_mimo(C.CHAIN_SPATIAL_CODED)   # Plan.coded, .mimo
    assert engine.chain_is_coded(C.CHAIN_SIMO_CODED) and not engine.chain_is_mimo(C.CHAIN_SIMO_CODED)
    assert engine.chain_is_mimo(C.CHAIN_SPATIAL) and not engine.chain_is_coded(C.CHAIN_SPATIAL)


def spatial_desc(C, **kw):
    d = C.PlanDesc()
    d.N, d.Nc, d.cp_len, d.bps, d.n_bits, d.max_frames = 128, 72, 9, 2, 435, 1
    d.chain, d.channel, d.num_tx, d.num_rx, d.rank, d.detector = C.CHAIN_SPATIAL_CODED, C.CH_AWGN, 2, 2, 2, C.DET_MMSE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_plan_create_refusals_without_a_device(C):
    """SIC: LTE_EUNSUP (soft SIC is not built); HARQ: LTE_EUNSUP; rank > num_rx:
    LTE_EINVAL -- each before the device is touched, alongside
    tests/test_capi_cpu.py's pattern."""
    lib = C.load()
    h = ctypes.c_void_p()
    d = spatial_desc(C, detector=C.DET_SIC)
    assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EUNSUP
    assert b'SIC' in lib.lte_last_error()
    d = spatial_desc(C)
    hd = C.HarqDesc()
    hd.max_tx = 4
    assert lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)) == C.LTE_EUNSUP
    assert b'HARQ' in lib.lte_last_error()
    d = spatial_desc(C, num_rx=1)
    assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EINVAL
    assert b'num_layers' in lib.lte_last_error()
    d = spatial_desc(C, detector=C.DET_MRC)                            # MRC is rank 1 only, as LTE_CHAIN_SPATIAL
    assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EINVAL
    d = spatial_desc(C, num_tx=3)                                      # 2 / 4 TX, as LTE_CHAIN_SPATIAL
    assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EUNSUP
    for ntx in (0, 1):                                                 # a multi-antenna chain on a one-antenna descriptor
        d = spatial_desc(C, num_tx=ntx)
        assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EINVAL
        assert b'bad chain for num_tx < 2' in lib.lte_last_error()
    d = spatial_desc(C, chain=9)                                       # the first unassigned value
    assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EINVAL
    assert lib.lte_last_error() == b'bad chain'


def test_python_entry_points():
    import lte_phy
    sig = inspect.signature(lte_phy.simulate_spatial_multiplexing_coded)
    assert list(sig.parameters) == ['bits', 'num_tx', 'num_rx', 'rank', 'detector_type', 'snr_db', 'config',
                                    'channel_type', 'itu_profile', 'velocity_kmh', 'frequency_ghz',
                                    'enable_csi_feedback', 'precision']
    assert sig.parameters['precision'].kind == inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError, match='cannot be empty'):
        lte_phy.simulate_spatial_multiplexing_coded([], 2, 2, 2, 'MMSE', 10.0)
    with pytest.raises(NotImplementedError, match='SIC'):             # before any plan (or device) is needed
        lte_phy.simulate_spatial_multiplexing_coded([0, 1, 1, 0], 2, 2, 2, 'SIC', 10.0)
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    with pytest.raises(NotImplementedError, match='SIC'):
        sim.run_grid([0.0], 1, coded=True, mimo='spatial', n_bits=435,
                     spatial={'num_tx': 2, 'num_rx': 2, 'rank': 2, 'detector': 'SIC'})
    assert len(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters) == 17      # no new keyword


def test_model_deinterleave_is_the_oracles(oracle):
    num = oracle.Numerology(bandwidth=5.0, modulation='16-QAM')
    perm, rows, total = oracle.tf_interleave_perm(1550, num.Nd)
    inv = np.empty(total, dtype=int)
    inv[perm] = np.arange(total)
    assert np.array_equal(M.deinterleave_index(1550, num.Nd), inv[:1550])


@pytest.mark.parametrize('name', list(M.CASES))
def test_ladder_case_straddles_the_cliff(oracle, mimo_oracle, tm4_oracle, name):
    """The model alone, 67 frames at 2 iterations: at least 8 frames pass their
    CRC and at least 8 fail, so the frames' decisions react to a wrong LLR."""
    inp, frames = M.case_frames(oracle, mimo_oracle, tm4_oracle, name)
    ok = [f['crc'] for f in frames]
    n_ok = sum(ok)
    print(f'spatial coded ladder {name}: {n_ok} pass / {M.FRAMES - n_ok} fail over {M.CASES[name]["snr"]} dB')
    assert len(ok) == M.FRAMES == 67
    assert n_ok >= M.MIN_PASS and M.FRAMES - n_ok >= M.MIN_FAIL, (name, n_ok)
    assert all((f['errs'] == 0) == f['crc'] for f in frames)    # (no CRC false alarm in the ladder)


def test_ladder_shapes(oracle):
    """The shapes the ladder is there for: a partly filled last subcarrier (Nd no
    multiple of the rank: R44, Z42, D22, C44 -- not R43, whose Nd = 249 = 3 * 83),
    N = 1024 (D22) and N = 2048 (C44)."""
    part = {n: M.numerology(oracle, cs).Nd % cs['rank'] for n, cs in M.CASES.items()}
    assert part == {'P22': 0, 'M21': 0, 'R44': 1, 'R43': 0, 'Z42': 1, 'D22': 1, 'C44': 3}
    assert M.numerology(oracle, M.CASES['D22']).N == 1024
    assert M.numerology(oracle, M.CASES['C44']).N == 2048


def test_model_stays_finite_at_the_clamps():
    """MMSE with mu clamped (a channel far below the noise: e_l reaches 1) and
    with a zero column (an undetectable layer): both evaluations stay finite,
    the zero column's estimate is 0 and nv stays within e / mu <= 1e6."""
    rs = np.random.RandomState(5)
    He = (rs.randn(6, 2, 2) + 1j * rs.randn(6, 2, 2)) * np.array([1.0, 1e-9, 1e-9, 1.0, 1e-200, 1.0])[:, None, None]
    He[3:5, :, 1] = 0.0                                                # a zero column; He[4] is all but zero
    y = rs.randn(6, 2) + 1j * rs.randn(6, 2)
    for rule in (M.soft_rule, M.soft_rule_chol):
        out = rule(He, y, 0.5, 'MMSE')
        z, nv = out[0], out[1]
        assert np.all(np.isfinite(z)) and np.all(np.isfinite(nv)) and np.all(nv > 0) and np.all(nv <= 1e6)
        assert np.all(z[3:5, 1] == 0) and np.allclose(nv[[1, 2, 4]], 1e6, rtol=1e-9, atol=0)
    assert list(out[0].shape) == [6, 2]
    kappa, mu_min = M.soft_rule(He, y, 0.5, 'MMSE')[2:]
    assert mu_min[[1, 2, 3, 4]].tolist() == [1e-6] * 4 and np.all(kappa >= 1.0) and np.all(np.isfinite(kappa))


def test_tolerance_measurement(oracle, mimo_oracle, tm4_oracle):
    """r_cpu: the soft rule evaluated a second way in NumPy (Cholesky, L^-1,
    diagonal: the kernel's order) against np.linalg.inv, over every subcarrier of
    the ladder, the worst of |dz| / (2^-52 kappa / mu_min ||z||) and |dLLR| /
    (2^-52 kappa / mu_min (1 + |LLR|)).  spatial_coded_model.R_CPU holds it."""
    per = {name: M.tolerance_ratio(oracle, mimo_oracle, tm4_oracle, name) for name in M.CASES}
    r_cpu = max(per.values())
    print('spatial coded r_cpu per case: ' + ', '.join(f'{k} {v:.6g}' for k, v in per.items()) +
          f'; r_cpu = {r_cpu:.9g} (R_CPU = {M.R_CPU})')
    assert r_cpu <= M.R_CPU, (r_cpu, M.R_CPU)
    assert r_cpu >= 0.5 * M.R_CPU, (r_cpu, M.R_CPU)                    # the constant is the measurement, not a cushion
