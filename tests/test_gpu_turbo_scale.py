"""GPU: extrinsic scaling of the turbo decoders (k_turbo64_sc / k_turbo_sc and
k_turbo64_es_sc / k_turbo_es_sc) against the models of
tests/turbo_scaled_model.py -- the oracle's decoders with the one multiply
e = s * ((L - La) - Ls) of include/lte_phy.h.

  (1) the stage entries of the fixed decoders, both precisions, two scales,
      1 / 2 / 8 iterations, 131 lanes per K (and 2117 lanes once: the wide
      chunk's instances)
  (2) the early-stop stage entries follow the rule on the scaled model, both
      generators and precisions; with re-packing (after = 1, 2, 3) the outputs
      are those of after = 0 and info is the model's count at the boundary
  (3) scale 1 is the unscaled decoder, and the path names the scale
  (4) the coded chains: the run's own captured LLRs through the model
  (5) HARQ: the rounds' combined soft rows through the model, skip on and off
  (6) run_grid with OFDMSimulator.turbo_scale, channel_coding.turbo_decode_scaled
  (7) refusals
Every comparison is exact.  The pools' conditions (a kernel that ignored the
scale cannot pass) are checked on the CPU in tests/test_turbo_scale_host.py."""
import numpy as np
import pytest

import harq_model as H
import turbo_scaled_model as M

pytestmark = pytest.mark.gpu

ITERS, NCB, POLYS = M.ITERS, M.NCB, M.POLYS
FRAMES = 64 + 3


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


@pytest.fixture(scope='module')
def cc(C):
    from lte_phy import channel_coding
    return channel_coding


# ---------------------------------------------------------------------------
# (1) stage entries, fixed decoders
FIXED = [(K, prec, s) for K in sorted(M.STAGE) for prec in ('f64', 'f32') for s in M.SCALES[prec == 'f32']]


@pytest.mark.parametrize('K,prec,scale', FIXED)
def test_fixed_decoder_equals_the_model(C, oracle, K, prec, scale):
    """131 lanes: one full wave, a second full wave, a partial third (three
    groups: the chunk-width-1 instances)."""
    f32 = prec == 'f32'
    llr, D, _, _ = M.stage_pool(oracle, K, '24B', f32, scale)
    D1 = M.stage_pool(oracle, K, '24B', f32, 1.0)[1]
    lanes = np.arange(NCB) % len(llr)
    for iters in (1, 2, 8):
        assert (D[:, iters] != D1[:, iters]).any()                 # the scale shows in the model's decisions
        bits = C.turbo_decode_scaled(llr[lanes], K, iters, scale, prec)
        bad = np.flatnonzero((bits != D[lanes, iters]).any(axis=1))
        assert np.array_equal(bits, D[lanes, iters]), (K, prec, scale, iters, bad.tolist())


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_wide_arrays(C, oracle, prec):
    """33 groups and a partial one: the chunk-width-TURBO_CH instances of the
    four scaled kernels (the decoder rows are chunked from 32 groups on)."""
    K, f32, scale = 40, prec == 'f32', M.ES_SCALE
    llr, D, n_star, _ = M.stage_pool(oracle, K, '24B', f32, scale)
    lanes = (7 * np.arange(33 * 64 + 5)) % len(llr)
    bits = C.turbo_decode_scaled(llr[lanes], K, ITERS, scale, prec)
    assert np.array_equal(bits, D[lanes, ITERS])
    for after in (0, 2):
        bits, used, info = C.turbo_decode_es_scaled(llr[lanes], K, ITERS, POLYS['24B'], scale, after, prec)
        assert np.array_equal(used, n_star[lanes]) and np.array_equal(bits, D[lanes, n_star[lanes]])


# ---------------------------------------------------------------------------
# (2) stage entries, early stop
def boundary_info(O, D, lanes, poly, after):
    """lte_turbo_decode_es_repack_host64's info [3] from the model: the lanes
    undecided after the check of D(after), the groups that run the rest, and
    none / packed / in place (packed arrays of max(1, ceil(G / 4)) groups)."""
    und = np.array([M.undecided_after(O, d, poly, after) for d in D])
    u, n = int(und[lanes].sum()), len(lanes)
    G = -(-n // 64)
    cap = -(-G // 4) if G > 4 else 1
    if u == 0:
        return [0, 0, 0]
    pack = u <= cap * 64 and u < n
    return [u, -(-u // 64) if pack else G, 1 if pack else 2]


@pytest.mark.parametrize('crc', ['24A', '24B'])
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('K', sorted(M.STAGE))
def test_early_stop_follows_the_rule_on_the_scaled_model(C, oracle, K, prec, crc):
    f32, scale = prec == 'f32', M.ES_SCALE
    llr, D, n_star, passed = M.stage_pool(oracle, K, crc, f32, scale)
    lanes = M.stage_lanes(passed)
    assert M.mixing(n_star[lanes], passed[lanes])
    want = D[lanes, n_star[lanes]]
    bits, used, info = C.turbo_decode_es_scaled(llr[lanes], K, ITERS, POLYS[crc], scale, 0, prec)
    assert info is None and used.dtype == np.uint8 and bits.shape == (NCB, K)
    assert np.array_equal(used, n_star[lanes]), (K, prec, crc, used.tolist(), n_star[lanes].tolist())
    assert np.array_equal(bits, want), (K, prec, crc, np.flatnonzero((bits != want).any(axis=1)).tolist())
    seen = set()
    for after in (1, 2, 3):
        b2, u2, info = C.turbo_decode_es_scaled(llr[lanes], K, ITERS, POLYS[crc], scale, after, prec)
        assert np.array_equal(b2, bits) and np.array_equal(u2, used), (K, prec, crc, after)
        assert info.tolist() == boundary_info(oracle, D, lanes, POLYS[crc], after), (K, prec, crc, after, info)
        seen.add(int(info[2]))
    assert seen & {1, 2}                                           # some boundary leaves blocks to resume


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('iters', [0, 1, 3])
def test_early_stop_iteration_limits(C, oracle, iters, prec):
    K, f32, scale = 56, prec == 'f32', M.ES_SCALE
    llr, D, _, _ = M.stage_pool(oracle, K, '24B', f32, scale)
    lanes = np.arange(NCB) % len(llr)
    ref = [M.rule(oracle, None, K, iters, POLYS['24B'], D=d[:iters + 1]) for d in D]
    bits, used, _ = C.turbo_decode_es_scaled(llr[lanes], K, iters, POLYS['24B'], scale, 0, prec)
    assert np.array_equal(used, np.array([r[1] for r in ref])[lanes])
    assert np.array_equal(bits, np.array([r[0] for r in ref])[lanes])


# ---------------------------------------------------------------------------
# (3) scale 1
def siso_sim(prec='f64', bw=1.25, mod='QPSK', chan='awgn', scale=None):
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=bw, modulation=mod), channel_type=chan, precision=prec)
    if scale is not None:
        sim.turbo_scale = scale
    return sim


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_scale_one_is_the_unscaled_decoder(C, cc, oracle, prec):
    K, f32 = 56, prec == 'f32'
    llr, D1, n1, passed = M.stage_pool(oracle, K, '24B', f32, 1.0)
    lanes = M.stage_lanes(passed)
    plain = cc.turbo_decode_batch(llr[lanes], K, ITERS, prec)
    assert np.array_equal(C.turbo_decode_scaled(llr[lanes], K, ITERS, 1.0, prec), plain)
    assert np.array_equal(plain, D1[lanes, ITERS])
    b0, u0 = cc.turbo_decode_early_stop(llr[lanes], K, ITERS, '24B', precision=prec)
    b1, u1, _ = C.turbo_decode_es_scaled(llr[lanes], K, ITERS, POLYS['24B'], 1.0, 0, prec)
    assert np.array_equal(b0, b1) and np.array_equal(u0, u1)
    b2, u2, info = C.turbo_decode_es_scaled(llr[lanes], K, ITERS, POLYS['24B'], 1.0, 2, prec)
    assert np.array_equal(b0, b2) and np.array_equal(u0, u2) and info[0] > 0


def test_path_names_the_scale(C):
    sim = siso_sim()
    plan = sim._plan(C.CHAIN_CODED, 0, 435, max_frames=4, iters=2)
    assert plan.turbo_scale == 1.0
    before = plan.path([3.0])
    plan.set_turbo_scale(1.0)
    assert plan.path([3.0]) == before and 'ext' not in before
    buf = np.zeros(256, dtype=np.uint8)

    def line():
        a, _, keep = plan._args([3.0])
        import ctypes
        n = C.load().lte_run_path(plan.h, ctypes.byref(a), buf.ctypes.data_as(ctypes.c_char_p), len(buf))
        return bytes(buf[:n]).decode()

    plain = line()
    try:
        plan.set_turbo_scale(0.75)
        assert plan.turbo_scale == 0.75 and C.load().lte_plan_turbo_scale(plan.h) == 0.75
        assert line() == plain + ' ext=0.75' and plan.path([3.0])['ext'] == '0.75'
        plan.set_turbo_scale(0.6875)
        assert line().endswith(' ext=0.6875')
        for bad in (0.0, -0.5, 1.0000001, float('nan'), float('inf')):
            assert C.load().lte_plan_set_turbo_scale(plan.h, bad) == C.LTE_EINVAL
            assert plan.turbo_scale == 0.6875
    finally:
        plan.set_turbo_scale(None)                                 # the cached plan goes back as it came
    assert line() == plain
    # a plan made with the keyword is another plan, and carries the scale
    scaled = siso_sim(scale=0.75)._plan(C.CHAIN_CODED, 0, 435, max_frames=4, iters=2)
    assert scaled is not plan and scaled.turbo_scale == 0.75 and plan.turbo_scale == 1.0
    # either order with the early-stop setters: the scale first, then early stop and re-packing ...
    lib = C.load()
    try:
        assert lib.lte_plan_set_early_stop(scaled.h, 1) == C.LTE_OK
        assert lib.lte_plan_set_early_stop_repack(scaled.h, 1) == C.LTE_OK
        assert lib.lte_plan_turbo_scale(scaled.h) == 0.75
        p = scaled._path(scaled._args([3.0])[0])
        assert (p['turbo'], p['repack'], p['ext']) == ('es', '1', '0.75')
    finally:
        assert lib.lte_plan_set_early_stop(scaled.h, 0) == C.LTE_OK
    assert scaled.path([3.0]) == dict(before, ext='0.75')
    # ... and the keywords' order: early stop and re-packing first, then the scale
    es = siso_sim(scale=0.75)._plan(C.CHAIN_CODED, 0, 435, max_frames=4, iters=4, early_stop=True, repack=1)
    p = es.path([3.0])
    assert (p['turbo'], p['repack'], p['ext']) == ('es', '1', '0.75') and list(p)[-1] == 'ext'


# ---------------------------------------------------------------------------
# (4) plans.  case -> (bandwidth, modulation, chain, TB bits, SNR range of frames 0..63); frames 64..66 run
# at the top SNR.  435: one code block (K = 464); 6121: 3072 + 3136, so the early-stop plans check gCRC24B.
SCALE = 0.75
PLAN_ITERS = 2
CASES = {
    'siso-435': (1.25, 'QPSK', 'siso', 435, (-1.0, 5.0)),
    'siso-6121': (5.0, '16-QAM', 'siso', 6121, (10.5, 16.5)),
    'sfbc-435': (1.25, 'QPSK', 'sfbc', 435, (-5.0, 3.0)),
    'simo-435': (1.25, 'QPSK', 'simo', 435, (-3.0, 4.0)),
    'spatial-435': (1.25, 'QPSK', 'spatial', 435, (0.0, 25.0)),
    'scfdm-435': (1.25, 'QPSK', 'scfdm', 435, (-1.0, 6.0)),
}
PLAN_CASES = [('siso-435', 'f64', 0, 0), ('siso-435', 'f32', 0, 0), ('siso-6121', 'f64', 0, 0),
              ('siso-6121', 'f32', 0, 0), ('sfbc-435', 'f64', 0, 0), ('simo-435', 'f64', 0, 0),
              ('spatial-435', 'f64', 0, 0), ('scfdm-435', 'f64', 0, 0),
              ('siso-435', 'f64', 1, 0), ('siso-6121', 'f64', 1, 0), ('siso-6121', 'f64', 1, 1),
              ('siso-6121', 'f32', 1, 1)]


def case_plan(C, case, prec, early_stop, repack, scale=SCALE):
    bw, mod, chain, n_bits, _ = CASES[case]
    sim = siso_sim(prec, bw, mod, scale=scale)
    kw = dict(max_frames=FRAMES, iters=PLAN_ITERS, early_stop=bool(early_stop), repack=repack or None)
    if chain == 'sfbc':
        return sim._sfbc_plan(0, n_bits, 2, coded=True, **kw)
    if chain == 'spatial':
        import lte_phy
        from lte_phy import ofdm_core
        from lte_phy.tm4 import DETECTORS, LTECodebook
        W = LTECodebook(2, transmission_mode='TM4', rank=2).get_precoder(0)
        return ofdm_core._spatial_plan(lte_phy.LTEConfig(bandwidth=bw, modulation=mod), 'awgn', 'Pedestrian_A', 0.0,
                                       2.0, 0, n_bits, FRAMES, num_tx=2, num_rx=2, rank=2, detector=DETECTORS['MMSE'],
                                       W=W, precision=prec, coded=True, turbo_iters=PLAN_ITERS,
                                       early_stop=bool(early_stop), repack=repack or None, turbo_scale=scale)[0]
    if chain == 'simo':
        return sim._plan(C.CHAIN_SIMO_CODED, 0, n_bits, num_rx=2, **kw)
    if chain == 'scfdm':
        return sim._plan(C.CHAIN_SCFDM_CODED, 0, n_bits, detector=sim._scfdm_equalizer('mmse')[1], **kw)
    return sim._plan(C.CHAIN_CODED, 0, n_bits, **kw)


def coded_order(plan, bps, llr_re):
    """A captured LLR array (grid order) in coded-bit order: the T/F interleaver
    of the coded chains with as many columns as an OFDM symbol carries QAM
    symbols (plan.res)."""
    coded, cols = plan.coded_bits, plan.res
    ncs = coded // bps
    rows = -(-ncs // cols)
    q = np.arange(ncs)
    return llr_re.astype(np.float64).reshape(-1, bps)[(q % cols) * rows + q // cols].reshape(-1)[:coded]


@pytest.mark.parametrize('case,prec,early_stop,repack', PLAN_CASES)
def test_plan_equals_the_model_on_its_own_llrs(C, oracle, case, prec, early_stop, repack):
    O = oracle
    bw, mod, chain, n_bits, (lo, hi) = CASES[case]
    plan = case_plan(C, case, prec, early_stop, repack)
    assert plan.turbo_scale == SCALE and plan.coded
    seg = O.segmentation_plan(n_bits + 24)
    rm = [3 * s[0] + 12 for s in seg]
    assert plan.n_cb == len(seg) == (1 if n_bits == 435 else 2) and plan.coded_bits == sum(rm)
    bps = O.Numerology(bandwidth=bw, modulation=mod).bps
    bits = np.random.RandomState(n_bits).randint(0, 2, (FRAMES, n_bits)).astype(np.uint8)
    snrs = np.concatenate([np.linspace(lo, hi, 64), np.full(FRAMES - 64, hi)])
    r = plan.run(snrs, seed=n_bits + 1, bits=bits, capture=('llr', 'bits_rx'))
    assert r.path['ext'] == '0.75' and r.path['dematch'] == 'llr'
    assert ('turbo' in r.path) == bool(early_stop) and ('repack' in r.path) == bool(repack)
    oks, differs = [], 0
    for b in range(FRAMES):
        L = coded_order(plan, bps, r['llr'][b])
        dec, ok, ns, _ = M.coded_rx_decode(O, L, seg, rm, PLAN_ITERS, SCALE, prec == 'f32', bool(early_stop))
        assert np.array_equal(dec, r['bits_rx'][b]), (case, prec, b, int(np.sum(dec != r['bits_rx'][b])))
        assert bool(ok) == bool(r['crc_ok'][b]), (case, prec, b)
        assert int(r['frame_errors'][b]) == int(np.sum(bits[b] != dec)), (case, prec, b)
        if early_stop:
            assert r['turbo_iters_used'][b].tolist() == ns, (case, prec, b)
        oks.append(bool(ok))
        plain = M.coded_rx_decode(O, L, seg, rm, PLAN_ITERS, 1.0, prec == 'f32', bool(early_stop))[0]
        differs += not np.array_equal(plain, dec)
    print(f'{case} {prec} es={early_stop} repack={repack}: {sum(oks)} pass / {FRAMES - sum(oks)} fail, '
          f'{differs} frames differ from the unscaled model')
    assert sum(oks) >= 8 and FRAMES - sum(oks) >= 8, (case, prec, sum(oks))
    assert differs >= 3                                            # a decoder without the multiply fails above
    want = np.array([[int(r['frame_errors'].sum()), FRAMES * n_bits, FRAMES - sum(oks), FRAMES]], dtype=np.uint64)
    assert np.array_equal(r['counts'], want)
    if repack:
        assert r['repack_info']['after'] == repack


# ---------------------------------------------------------------------------
# (5) HARQ
class ScaledOracle:
    """The oracle with its two decoders replaced by the scaled models'."""

    def __init__(self, O, scale):
        self._O, self._s = O, scale

    def __getattr__(self, name):
        return getattr(self._O, name)

    def turbo_decode(self, llr, K, iters):
        return M.turbo_decode_scaled(self._O, llr, K, iters, self._s)

    def turbo_decode_f32_model(self, llr, K, iters):
        return M.turbo_decode_scaled(self._O, llr, K, iters, self._s, True)


HQ_TX, HQ_RV, HQ_NB, HQ_G = 3, (0, 2, 3), 435, 766      # (435 + 24) / 766: rate 0.6


def test_harq_rounds_equal_the_model(C, oracle, monkeypatch):
    """197 frames as tests/test_gpu_harq.py groups them: a group at a high SNR
    (at rate 0.6 it is acknowledged with the second transmission and skipped in
    the third), a ladder group, a group that never finishes, a partial group."""
    O = oracle
    B = 197
    sim = siso_sim(scale=SCALE)
    harq = dict(max_tx=HQ_TX, rv_seq=HQ_RV, coded_bits=HQ_G)
    plan = sim._plan(C.CHAIN_CODED, 0, HQ_NB, max_frames=B, iters=PLAN_ITERS, harq=harq)
    assert plan.turbo_scale == SCALE
    num = O.Numerology(bandwidth=1.25, modulation='QPSK')
    Ks, Es = H.split(O, HQ_NB, num.bps, HQ_G)
    bits = np.random.RandomState(5).randint(0, 2, (B, HQ_NB)).astype(np.uint8)
    snrs = np.concatenate([np.full(64, 14.0), np.linspace(-1.0, 6.0, 64), np.full(64, -20.0), np.linspace(-1.0, 6.0, 5)])
    kw = dict(seed=9, bits=bits)
    monkeypatch.setenv('LTE_HARQ_SKIP', '1')
    on = plan.run_harq(snrs, capture=('llr', 'bits_rx'), **kw)
    monkeypatch.setenv('LTE_HARQ_SKIP', '0')
    off = plan.run_harq(snrs, capture=('bits_rx',), **kw)
    assert on.path['harq'].endswith('skip=1') and off.path['harq'].endswith('skip=0')
    assert on.path['ext'] == off.path['ext'] == '0.75'
    assert on['rounds_run'] == off['rounds_run'] == HQ_TX
    for k in ('tx_used', 'crc_ok', 'frame_errors', 'counts_by_round'):
        assert np.array_equal(on[k], off[k]), k
    assert off['skipped'] == [0] * HQ_TX and sum(on['skipped']) >= 1
    seg = O.segmentation_plan(HQ_NB + 24)
    proc = H.Process(ScaledOracle(O, SCALE), seg, Es, HQ_RV, bits, PLAN_ITERS)
    plain = H.Process(O, seg, Es, HQ_RV, bits, PLAN_ITERS)
    differs = 0
    for t in range(HQ_TX):
        llr = [H.llr_coded_order(on['rounds'][t]['llr'][b], num, sum(Es)) for b in range(B)]
        fin = proc.finished_groups() if t else []                  # what the skip leaves out of this round
        m, m1 = proc.round(t, llr), plain.round(t, llr)
        assert on['skipped'][t] == m['skipped'], (t, on['skipped'], m['skipped'])
        assert np.array_equal(on['rounds'][t]['bits_rx'], m['bits_rx']), t
        assert np.array_equal(on['counts_by_round'][t], proc.counts()), t
        differs += int(np.sum((m['bits_rx'] != m1['bits_rx']).any(axis=1)))
        # without the skip the finished groups are decoded again (their latched results stay); the other
        # groups' bits are the same decode
        live = np.array([b // 64 not in fin for b in range(B)])
        assert np.array_equal(off['rounds'][t]['bits_rx'][live], m['bits_rx'][live]), t
    for k in ('tx_used', 'crc_ok', 'frame_errors'):
        assert np.array_equal(on[k], m[k]), k
    hist = H.histogram(m['tx_used'], m['crc_ok'], HQ_TX)
    print('harq histogram [never, 1, 2, 3]:', hist, 'frames differing from the unscaled model:', differs)
    assert hist[0] >= 3 and sum(h >= 3 for h in hist[1:]) >= 2, hist   # never, and two acknowledgement classes
    assert differs >= 3


# ---------------------------------------------------------------------------
# (6) Python
GRID_SNRS = [2.0, 3.5, 4.0, 12.0]
GRID_T, GRID_NB, GRID_SEED = 6, 6200, 11


def grid_model_errors(O, scale):
    """[S][T] (bit errors, crc ok) of the run_grid frames through the oracle's
    front end and the model."""
    from oracle import philox as P
    num = O.Numerology(bandwidth=1.25, modulation='QPSK')
    out = []
    for s, snr in enumerate(GRID_SNRS):
        row = []
        for t in range(GRID_T):
            frame = s * GRID_T + t
            bits = P.payload_bits(GRID_SEED, frame, GRID_NB)
            tx = O.coded_tx(num, bits)
            draws = P.siso_draws(GRID_SEED, frame, len(tx['signal']), 0)
            rx = O.channel_transmit(num, tx['signal'], 'awgn', snr, 'Pedestrian_A', 0.0, draws[0])
            L = O.coded_rx_llrs(num, rx, len(tx['coded']), snr, 'awgn')[0]
            dec, ok, _, _ = M.coded_rx_decode(O, L, tx['plan'], tx['rm_lens'], ITERS, scale)
            row.append((int(np.sum(dec != bits)), bool(ok)))
        out.append(row)
    return out


def test_run_grid_honours_the_attribute(C, oracle):
    sim = siso_sim()
    kw = dict(seed=GRID_SEED, coded=True, n_bits=GRID_NB, frames_per_call=8)
    plain = sim.run_grid(GRID_SNRS, GRID_T, **kw)
    sim.turbo_scale = 0.75
    full = sim.run_grid(GRID_SNRS, GRID_T, **kw)
    parts = [sim.run_grid(GRID_SNRS, GRID_T, rank=k, world_size=2, **kw) for k in range(2)]
    assert full['plan'].turbo_scale == 0.75 and plain['plan'].turbo_scale == 1.0
    assert np.array_equal(parts[0]['counts'] + parts[1]['counts'], full['counts'])
    assert np.array_equal(full['counts'][:, 3], np.full(len(GRID_SNRS), GRID_T))
    # where the model says the scale must show: block errors per SNR differ between the two decoders
    blk = {s: np.array([sum(not ok for _, ok in row) for row in grid_model_errors(oracle, s)]) for s in (1.0, 0.75)}
    must = np.flatnonzero(blk[1.0] != blk[0.75])
    assert len(must) >= 1, (blk[1.0].tolist(), blk[0.75].tolist())
    assert not np.array_equal(full['counts'], plain['counts'])
    assert np.array_equal(full['counts'][:, 2], blk[0.75]) and np.array_equal(plain['counts'][:, 2], blk[1.0])
    sim.turbo_scale = 1.0
    assert np.array_equal(sim.run_grid(GRID_SNRS, GRID_T, **kw)['counts'], plain['counts'])


def test_turbo_decode_scaled(cc, oracle):
    K = 64
    llr, D, _, _ = M.stage_pool(oracle, K, '24B', False, 0.75)
    assert cc.turbo_decode_scaled.__defaults__ == (8, 0.75)
    one = cc.turbo_decode_scaled(llr[5], K)
    assert one.shape == (K,) and np.array_equal(one, D[5, 8])
    assert np.array_equal(cc.turbo_decode_scaled(llr, K, 8, 0.75), D[:, 8])
    D5 = M.stage_pool(oracle, K, '24B', False, 0.5)[1]
    assert np.array_equal(cc.turbo_decode_scaled(llr, K, 2, scale=0.5), D5[:, 2])
    assert np.array_equal(cc.turbo_decode_scaled(llr, K, 8, 1.0), cc.turbo_decode_batch(llr, K, 8))
    with pytest.raises(ValueError, match='turbo_scale'):
        cc.turbo_decode_scaled(llr, K, 8, 1.5)


# ---------------------------------------------------------------------------
# (7) refusals
def test_uncoded_plans_refuse_the_scale(C):
    sim = siso_sim()
    plan = sim._plan(C.CHAIN_UNCODED, 14, 14 * sim.Nd * 2, max_frames=4)
    assert C.load().lte_plan_set_turbo_scale(plan.h, 0.75) == C.LTE_EINVAL
    assert C.load().lte_plan_set_turbo_scale(plan.h, 1.0) == C.LTE_EINVAL
    assert plan.turbo_scale == 1.0
    sim.turbo_scale = 0.75                                         # the uncoded drivers do not pass it on
    assert sim._plan(C.CHAIN_UNCODED, 14, 14 * sim.Nd * 2, max_frames=4) is plan


def test_exact_logmap_refuses_the_scale(C, cc, oracle):
    plan = siso_sim(scale=0.75)._plan(C.CHAIN_CODED, 0, 435, max_frames=4, iters=2)
    bits = np.random.RandomState(0).randint(0, 2, (4, 435)).astype(np.uint8)
    snrs = np.full(4, 6.0)
    llr = M.stage_pool(oracle, 40, '24A', False, 0.75)[0]
    l32 = llr.astype(np.float32)
    out, used = np.zeros((len(llr), 40), dtype=np.uint8), np.zeros(len(llr), dtype=np.uint8)
    lib = C.load()
    try:
        cc.set_decoder_mode(False)
        with pytest.raises(NotImplementedError, match='max-log'):       # LTE_EUNSUP (_capi.check)
            plan.run(snrs, seed=1, bits=bits)
        with pytest.raises(NotImplementedError, match='max-log'):
            cc.turbo_decode_scaled(llr, 40, ITERS, 0.75)
        assert lib.lte_turbo_decode_scaled_host64(40, 2, len(llr), C.ptr(llr, C.F64), 0.75,
                                                  C.ptr(out, C.U8)) == C.LTE_EUNSUP
        assert lib.lte_turbo_decode_scaled_host(40, 2, len(llr), C.ptr(l32, C.F32), 0.75,
                                                C.ptr(out, C.U8)) == C.LTE_EUNSUP
        assert lib.lte_turbo_decode_es_scaled_host64(40, 2, len(llr), C.ptr(llr, C.F64), POLYS['24A'], 0.75, 0,
                                                     C.ptr(out, C.U8), C.ptr(used, C.U8), None) == C.LTE_EUNSUP
        # scale 1 under the exact mode is the unscaled entry: the log-MAP decode
        assert np.array_equal(C.turbo_decode_scaled(llr, 40, 2, 1.0, 'f64'), cc.turbo_decode_batch(llr, 40, 2))
    finally:
        cc.set_decoder_mode(True)
    assert plan.run(snrs, seed=1, bits=bits)['crc_ok'].all()            # and runs again in max-log mode
