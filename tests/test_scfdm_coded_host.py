"""CPU: the interface of the coded SC-FDM chain (LTE_CHAIN_SCFDM_CODED: DFT
precoder, soft MMSE / ZF frequency-domain equaliser, turbo coding) -- the header
line, the ctypes constant, the checks lte_plan_create makes before the device is
touched, the Python entry points' signatures, and the model of
tests/scfdm_coded_model.py on its own: every ladder case of
tests/test_gpu_scfdm_coded.py straddles the turbo cliff; the two rules coincide
on a flat channel; the rule stays finite where it clamps; ZF's weights are the
coded SIMO combiner's output; and R_CPU, the unit of the GPU tests' bars, is
measured here.  The kernels are checked on the GPU in
tests/test_gpu_scfdm_coded.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import scfdm_coded_model as M
import simo_coded_model as SM


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def test_header_and_binding_name_the_chain(C):
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    assert re.search(r'^\s*LTE_CHAIN_SCFDM_CODED = 9$', text, re.M)
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)      # an additive value: no new version
    assert C.CHAIN_SCFDM_CODED == 9 and C.load().lte_version() == 3 and C.ABI_VERSION == 3
    from lte_phy import engine
    assert engine.chain_is_coded(9) and not engine.chain_is_mimo(9)  # Plan.coded, Plan.mimo: one TX, SISO captures
    assert engine.chain_is_coded(C.CHAIN_CODED) and not engine.chain_is_coded(C.CHAIN_UNCODED)


def scfdm_desc(C, **kw):
    d = C.PlanDesc()
    d.N, d.Nc, d.cp_len, d.bps, d.n_bits, d.max_frames = 128, 72, 9, 2, 435, 1
    d.chain, d.channel, d.num_rx = C.CHAIN_SCFDM_CODED, C.CH_AWGN, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_plan_create_refusals_without_a_device(C):
    """Each of the chain's refusals, answered before the device is touched."""
    lib = C.load()
    h = ctypes.c_void_p()

    def create(**kw):
        d = scfdm_desc(C, **kw)
        return lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)), lib.lte_last_error()

    for det in (C.DET_SIC, C.DET_MRC, 7, -1):                          # MMSE (0: a zeroed descriptor) and ZF only
        rc, msg = create(detector=det)
        assert rc == C.LTE_EINVAL and b'detector' in msg and str(det).encode() in msg, (det, msg)
    for nrx in (0, 9, 16, 17):
        rc, msg = create(num_rx=nrx)
        assert rc == C.LTE_EUNSUP and b'RX' in msg, (nrx, msg)
    for ntx in (2, 4):                                                 # a one-TX chain
        rc, msg = create(num_tx=ntx)
        assert rc == C.LTE_EINVAL and msg == b'bad chain', (ntx, msg)
    rc, msg = create(chain=10)                                         # the first unassigned value
    assert rc == C.LTE_EINVAL and msg == b'bad chain'
    rc, msg = create(chain=-1)
    assert rc == C.LTE_EINVAL and msg == b'bad chain'
    d, hd = scfdm_desc(C), C.HarqDesc()
    hd.max_tx = 4
    assert lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)) == C.LTE_EUNSUP
    assert b'HARQ' in lib.lte_last_error()
    # the chain passes the chain-range check: with valid fields the next refusal is a later one
    rc, msg = create(n_bits=0)
    assert rc == C.LTE_EINVAL and b'empty' in msg, msg
    for nrx, det in ((1, C.DET_MMSE), (8, C.DET_ZF)):
        rc, msg = create(num_rx=nrx, detector=det, max_frames=0)
        assert rc == C.LTE_EINVAL and b'max_frames' in msg, msg


def test_python_entry_points():
    import lte_phy
    sim_sig = inspect.signature(lte_phy.OFDMSimulator.simulate_scfdm_coded)
    got = [(p.name, p.default) for p in sim_sig.parameters.values()][1:]
    assert got == [('bits', inspect.Parameter.empty), ('snr_db', 10.0), ('num_rx', 1), ('equalizer', 'mmse')]
    grid_sig = inspect.signature(lte_phy.OFDMSimulator.run_scfdm_grid)
    got = [(p.name, p.default) for p in grid_sig.parameters.values()][1:]
    assert got == [('snr_range', inspect.Parameter.empty), ('num_trials', inspect.Parameter.empty), ('seed', 0),
                   ('num_rx', 1), ('equalizer', 'mmse'), ('n_bits', None), ('frames_per_call', 4096), ('rank', 0),
                   ('world_size', 1), ('turbo_iters', 8), ('early_stop', False)]
    assert len(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters) == 17      # no new keyword
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    with pytest.raises(ValueError, match='cannot be empty'):           # each before any plan (or device) is needed
        sim.simulate_scfdm_coded([], 5.0)
    with pytest.raises(ValueError, match='num_rx must be >= 1'):
        sim.simulate_scfdm_coded([0, 1, 1, 0], 5.0, num_rx=0)
    with pytest.raises(ValueError, match='equalizer'):
        sim.simulate_scfdm_coded([0, 1, 1, 0], 5.0, equalizer='sic')
    with pytest.raises(ValueError, match='equalizer'):
        sim.run_scfdm_grid([0.0], 1, equalizer='mrc')


def test_ladder_shapes(oracle):
    """The shapes the ladder is there for: a slot of 16, 32, 64, 128 and 256
    threads, both rules, 1 / 2 / 5 RX, and (B1L) three code blocks in 38 OFDM
    symbols = 3 estimation groups with a zero-padded last symbol."""
    N = {n: M.numerology(oracle, cs).N for n, cs in M.CASES.items()}
    assert N == {'A1M': 128, 'A2Z': 128, 'E1M': 256, 'B1M': 512, 'B1Z': 512, 'B5M': 512, 'B1L': 512, 'D2M': 1024,
                 'C1M': 2048, 'C1Z': 2048}
    assert {(cs['eq'], cs['nrx']) for cs in M.CASES.values()} == {('mmse', 1), ('zf', 2), ('zf', 1), ('mmse', 5),
                                                                  ('mmse', 2)}
    cs = M.CASES['B1L']
    num = M.numerology(oracle, cs)
    tx = M.coded_tx(oracle, num, np.zeros(cs['n_bits'], dtype=np.int64))
    assert len(tx['plan']) == 3 and tx['n_ofdm'] == 38 and len(tx['qam']) % num.Nd != 0
    assert tx['n_ofdm'] * num.Nd - len(tx['qam']) >= 1                  # zeros on the grid, precoded like symbols


def test_model_tx_is_the_coded_chains_with_the_precoder(oracle):
    """coded_tx restates oracle.coded_tx step by step: the same coded bits, QAM
    symbols and grid, and the signal of the oracle's uncoded SC-FDM modulator's
    steps (dft_matrix per symbol, then ofdm_symbols_tx)."""
    cs = M.CASES['A1M']
    num = M.numerology(oracle, cs)
    bits = np.random.RandomState(1).randint(0, 2, cs['n_bits'])
    a, b = M.coded_tx(oracle, num, bits), oracle.coded_tx(num, bits)
    assert np.array_equal(a['coded'], b['coded']) and np.array_equal(a['qam'], b['qam'])
    assert a['rm_lens'] == b['rm_lens'] and a['n_ofdm'] == b['n_ofdm'] and len(a['signal']) == len(b['signal'])
    F = oracle.dft_matrix(num.Nd)
    want = oracle.ofdm_symbols_tx(num, np.stack([F @ r for r in a['grid']]), oracle.pilots(0, num.Np))
    assert np.array_equal(a['signal'], want) and not np.allclose(a['signal'], b['signal'])
    src = M.deinterleave_index(len(a['qam']), num.Nd)
    assert np.array_equal(a['grid'].reshape(-1)[src], a['qam'])


@pytest.mark.parametrize('name', list(M.CASES))
def test_ladder_case_straddles_the_cliff(oracle, name):
    """The model alone, 67 frames at 2 iterations: at least 8 frames pass their
    CRC and at least 8 fail, so the frames' decisions react to a wrong LLR."""
    inp, frames = M.case_frames(oracle, name)
    ok = [f['crc'] for f in frames]
    n_ok = sum(ok)
    print(f'scfdm coded ladder {name}: {n_ok} pass / {M.FRAMES - n_ok} fail over {M.CASES[name]["snr"]} dB')
    assert len(ok) == M.FRAMES == 67
    assert n_ok >= M.MIN_PASS == 8 and M.FRAMES - n_ok >= M.MIN_FAIL == 8, (name, n_ok)
    assert all((f['errs'] == 0) == f['crc'] for f in frames)    # (no CRC false alarm in the ladder)


@pytest.mark.parametrize('name', list(M.CASES))
def test_ladder_decisions_survive_the_models_own_spread(oracle, name):
    """The GPU test holds a float64 run to the model's own decisions, so these
    must not hang on the model's round-off: the rule evaluated the second way
    (soft_rule_kernel_order) decodes to the same bits in every frame, failing
    frames included."""
    cs = M.CASES[name]
    num = M.numerology(oracle, cs)
    _, frames = M.case_frames(oracle, name)
    for f, (fr, (z2, nv2)) in enumerate(zip(frames, M.second_evaluation(oracle, name))):
        L2 = M.soft_output(oracle, num, z2, nv2, len(fr['tx']['coded']))
        dec, ok = oracle.coded_rx_decode(L2, fr['tx']['plan'], fr['tx']['rm_lens'], M.ITERS)
        assert np.array_equal(dec, fr['bits_rx']) and bool(ok) == fr['crc'], (name, f)


def test_rules_coincide_on_a_flat_channel(oracle):
    """H constant over k: e / mu = s2 / |H|^2 = ZF's nv, and z is equal."""
    rs = np.random.RandomState(2)
    Nd = 62
    Finv = oracle.dft_matrix(Nd, inverse=True)
    for D0, s2 in ((1.0, 0.1), (0.37, 2.0), (5.0, 1e-3)):
        h = np.sqrt(D0) * np.exp(0.7j)
        x = rs.randn(Nd) + 1j * rs.randn(Nd)
        nm, D = np.conj(h) * (h * x), np.full(Nd, abs(h) ** 2)
        zm, nvm, mu = M.soft_rule(nm, D, s2, 'mmse', Finv)
        zz, nvz, one = M.soft_rule(nm, D, s2, 'zf', Finv)
        assert one == 1.0 and abs(mu - D0 / (D0 + s2)) < 1e-15
        assert abs(nvm / (s2 / D0) - 1) < 1e-13 and abs(nvz / (s2 / D0) - 1) < 1e-13
        # z: both are IDFT(x) to round-off, ZF's scaled by its 1e-10 regulariser's D / (D + 1e-10)
        assert np.max(np.abs(zm - Finv @ x)) < 1e-13 * np.linalg.norm(x)
        assert np.max(np.abs(zz * ((D0 + 1e-10) / D0) - zm)) < 1e-13 * np.linalg.norm(x)


def test_model_stays_finite_at_the_clamps(oracle):
    """D = 0 on some subcarriers; D << s2 everywhere, so that mu hits 1e-6; D =
    1e-200: z and nv stay finite and nv positive, in both evaluations."""
    rs = np.random.RandomState(5)
    N, Nd = 128, 62
    Finv = oracle.dft_matrix(Nd, inverse=True)
    tables = M.bluestein_tables(N, Nd)
    nm = rs.randn(Nd) + 1j * rs.randn(Nd)
    holes = np.abs(rs.randn(Nd)) + 0.1
    holes[[0, 7, 61]] = 0.0
    for D, s2 in ((holes, 0.5), (np.full(Nd, 1e-9), 0.5), (np.full(Nd, 1e-200), 0.5), (np.zeros(Nd), 1e-3)):
        nmD = nm * np.sqrt(D)                                          # |num| <= sqrt(D) |Y|
        for eq in ('mmse', 'zf'):
            for z, nv, mu in (M.soft_rule(nmD, D, s2, eq, Finv), M.soft_rule_kernel_order(nmD, D, s2, eq, N, tables)):
                assert np.all(np.isfinite(z)) and np.isfinite(nv) and nv > 0 and 1e-6 <= mu <= 1.0, (eq, s2)
            if eq == 'mmse' and D.max() < 1e-8:
                assert mu == 1e-6 and abs(nv / 1e6 - 1) < 1e-6
            if eq == 'zf' and D.max() < 1e-8:
                assert abs(nv / (s2 * 1e6) - 1) < 1e-12                # the clip at 1e-6


def test_zf_weights_are_the_simo_combiners_output(oracle):
    """One RX, 'zf': the pre-IDFT weights are simo_coded_model.combine's z on the
    same received stream, bit for bit."""
    cs = dict(M.CASES['B1Z'])
    num = M.numerology(oracle, cs)
    rs = np.random.RandomState(9)
    bits = rs.randint(0, 2, cs['n_bits'])
    tx = M.coded_tx(oracle, num, bits)
    dl, _ = M.taps(oracle, num, cs)
    draws = M.draws_of(2 * np.pi * rs.rand(1, len(dl), 16), rs.standard_normal((1, 2, len(tx['signal']))))
    rxs = [oracle.channel_transmit(num, tx['signal'], cs['chan'], 12.0, cs['prof'], 0.0, draws[0])]
    nm, D = M.mrc_sums(oracle, num, rxs)
    w = np.concatenate([M.weights(nm[l], D[l], 0.1, 'zf') for l in range(nm.shape[0])])
    assert np.array_equal(w, SM.combine(oracle, num, rxs)[0])


def test_slot_sum_is_a_sum_in_a_fixed_order():
    rs = np.random.RandomState(3)
    for N, Nd in ((128, 62), (256, 125), (512, 249), (1024, 499), (2048, 999)):
        v = rs.rand(Nd)
        assert abs(M.slot_sum(v, N) - np.sum(v)) < 1e-12 * np.sum(v)
        ints = np.arange(1.0, Nd + 1)                                  # exact in any order
        assert M.slot_sum(ints, N) == Nd * (Nd + 1) / 2


def test_tolerance_measurement(oracle):
    """r_cpu: the soft rule evaluated a second way in NumPy, in the kernel's
    order (Bluestein on N-point np.fft with the library's tables, slot_sum),
    against the dense IDFT matrix and np.mean, over every symbol of the ladder.
    scfdm_coded_model.R_CPU_Z / R_CPU_LLR hold the two measured worst ratios and
    R_CPU their maximum."""
    per = {name: M.tolerance_ratio(oracle, name) for name in M.CASES}
    rz, rl = max(v[0] for v in per.values()), max(v[1] for v in per.values())
    print('scfdm coded r_cpu (z, LLR) per case: ' + ', '.join(f'{k} {v[0]:.6g} {v[1]:.6g}' for k, v in per.items()) +
          f'; r_cpu = {max(rz, rl):.9g} (R_CPU = {M.R_CPU}), z alone {rz:.9g} (R_CPU_Z = {M.R_CPU_Z})')
    assert 0.5 * M.R_CPU_Z <= rz <= M.R_CPU_Z, (rz, M.R_CPU_Z)         # the constants are the measurement,
    assert 0.5 * M.R_CPU_LLR <= rl <= M.R_CPU_LLR, (rl, M.R_CPU_LLR)   # not a cushion
    assert M.R_CPU == max(M.R_CPU_Z, M.R_CPU_LLR) and 0.5 * M.R_CPU <= max(rz, rl) <= M.R_CPU
