"""GPU: CRC early termination of the turbo decoders (k_turbo64_es / k_turbo_es)
against the rule, evaluated with the oracle's fixed-iteration decoders.

The rule: with D(n) the decisions of a decode of n iterations
(oracle.turbo_decode, or oracle.turbo_decode_f32_model for the float32
kernels), a code block stops at n* = min { n in 1..iters : the CRC-24 remainder
of all K bits of D(n) is zero }, n* = iters if no n passes, n* = 0 for iters =
0; the decoder returns D(n*) and reports n*.  D(n*) is not always D(iters), so
nothing here compares with a fixed-iteration run of the early-stop plan.

  (1) the stage entries, both precisions and generators, 131 blocks per K: a
      first wave that mixes blocks stopping at different iterations with blocks
      that never pass, a second wave of passing blocks only (the wave-wide
      exit), a partial third wave
  (2) the coded chains (SISO and SFBC) over transport-block sizes with one,
      two and three code blocks: the oracle applies the rule to the run's own
      captured LLRs
  (3) a plan without the keyword is the fixed-iteration plan it always was
  (4) run_grid(early_stop=True): shards add up, histogram rows are complete
  (5) refusals
Every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 8
FRAMES = 64 + 3
NCB = 2 * 64 + 3
POLYS = {'24A': 0x1864CFB, '24B': 0x1800063}


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


@pytest.fixture(scope='module')
def cc(C):
    from lte_phy import channel_coding
    return channel_coding


def rule(O, llr, K, iters, poly, f32=False):
    """(D(n*), n*, passed) of one code block."""
    dec = O.turbo_decode_f32_model if f32 else O.turbo_decode
    d = dec(llr, K, 0)
    for n in range(1, iters + 1):
        d = dec(llr, K, n)
        if not O.crc_bits(d, poly, 24).any():   # crc(D) = D(x) x^24 mod g: zero iff g divides D(x)
            return d, n, True
    return d, iters, False


def mixing(n_star, passed):
    """The condition on the oracle's own n* without which a case proves nothing:
    lanes 0..63 hold at least three stopping iterations, one of them a block
    that never passes (so the wave runs to the end with finished lanes in it);
    every later lane passes (so its wave leaves early, all lanes done)."""
    n_star, passed = np.asarray(n_star), np.asarray(passed)
    return len(set(n_star[:64].tolist())) >= 3 and not passed[:64].all() and passed[64:].all() and \
        n_star[64:].max() < ITERS


# ---------------------------------------------------------------------------
# (1) stage entries
# K -> (ladder of per-block SNRs in dB, seed).  40: two words, the last one
# partial; 48, 56: 6 / 7 sub-windows (56: a remainder against the 24-step
# super-window); 64: whole words; 1056, 6144: many super-windows.  The
# reference's max-log decoder has its cliff near 3.5 dB on these LLRs.
# seed: moved (never the condition) until the pool meets `mixing` for both generators and precisions
STAGE = {40: (np.linspace(-1.0, 4.0, 47), 0), 48: (np.linspace(-1.0, 4.0, 47), 1),
         56: (np.linspace(-1.0, 4.0, 47), 1), 64: (np.linspace(-1.0, 4.0, 47), 0),
         1056: (np.linspace(2.0, 4.5, 11), 0), 6144: (np.linspace(2.75, 4.25, 7), 0)}
_POOL = {}


def stage_pool(O, K, crc, f32):
    """Distinct blocks of one K: random payload + CRC-24 (generator `crc`),
    turbo-encoded, BPSK LLRs 2y / s2 with y = 1 - 2c + sqrt(s2) randn at the
    block's own SNR, and last the all-zero word with strong LLRs (it passes:
    zero-init CRC).  Returns (llr [n][3K+12], D(n*), n*, passed)."""
    key = (K, crc, f32)
    if key not in _POOL:
        snrs, seed = STAGE[K]
        rs = np.random.RandomState(1000 * seed + K)
        llr = []
        for snr in snrs:
            p = rs.randint(0, 2, K - 24).astype(np.uint8)
            cb = np.concatenate([p, O.crc_bits(p, POLYS[crc], 24)])
            s2 = 10 ** (-snr / 10)
            y = 1 - 2.0 * O.turbo_encode(cb) + np.sqrt(s2) * rs.randn(3 * K + 12)
            llr.append(2 * y / s2)
        llr.append(np.full(3 * K + 12, 8.0))
        llr = np.array(llr, dtype=np.float32 if f32 else np.float64)
        res = [rule(O, l, K, ITERS, POLYS[crc], f32) for l in llr]
        _POOL[key] = (llr, np.array([r[0] for r in res]), np.array([r[1] for r in res]),
                      np.array([r[2] for r in res]))
    return _POOL[key]


def stage_lanes(passed):
    """Pool index of each of the NCB lanes: wave 0 every pool block in turn,
    wave 1 the passing ones only, then three more of any kind."""
    n = len(passed)
    ok = np.flatnonzero(passed)
    return np.concatenate([np.arange(64) % n, ok[np.arange(64) % len(ok)], ok[np.arange(3) % len(ok)]])


@pytest.mark.parametrize('crc', ['24A', '24B'])
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('K', sorted(STAGE))
def test_stage_entry_follows_the_rule(cc, oracle, K, prec, crc):
    f32 = prec == 'f32'
    llr, d, n_star, passed = stage_pool(oracle, K, crc, f32)
    lanes = stage_lanes(passed)
    assert passed[-1] and n_star[-1] == 1 and not d[-1].any()          # the all-zero word
    assert mixing(n_star[lanes], passed[lanes]), (K, prec, crc, n_star.tolist(), passed.tolist())
    bits, used = cc.turbo_decode_early_stop(llr[lanes], K, ITERS, crc, precision=prec)
    assert used.dtype == np.uint8 and bits.shape == (NCB, K)
    assert np.array_equal(used, n_star[lanes]), (K, prec, crc, used.tolist(), n_star[lanes].tolist())
    assert np.array_equal(bits, d[lanes]), (K, prec, crc, np.flatnonzero((bits != d[lanes]).any(axis=1)).tolist())


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('iters', [0, 1, 3])
def test_stage_entry_iteration_limits(cc, oracle, iters, prec):
    """iters = 0: no check, D(0) and n* = 0; 1: the final pass right after the
    first iteration, no check in between; 3: one checked iteration more."""
    K, f32 = 56, prec == 'f32'
    llr = stage_pool(oracle, K, '24B', f32)[0]
    lanes = np.arange(NCB) % len(llr)
    ref = [rule(oracle, l, K, iters, POLYS['24B'], f32) for l in llr]
    bits, used = cc.turbo_decode_early_stop(llr[lanes], K, iters, '24B', precision=prec)
    assert np.array_equal(used, np.array([r[1] for r in ref])[lanes])
    assert np.array_equal(bits, np.array([r[0] for r in ref])[lanes])
    assert not all(r[2] for r in ref) or iters == 0
    if iters > 1:
        assert len({r[1] for r in ref}) >= 2


def test_single_block_form(cc, oracle):
    llr, d, n_star, _ = stage_pool(oracle, 40, '24A', False)
    bits, used = cc.turbo_decode_early_stop(llr[5], 40, ITERS, '24A')
    assert bits.shape == (40,) and isinstance(used, int)
    assert used == n_star[5] and np.array_equal(bits, d[5])


# ---------------------------------------------------------------------------
# (2) the coded chains
# case -> (bandwidth, modulation, channel, chain, TB bits, (lowest, highest SNR) of frames 0..63, seed);
# frames 64..66 (the second, partial wave of every code-block slot) run at the top SNR + 6 dB.
# TB 1: K = 40 with 15 fillers, CRC-24A is the block's CRC; 6120: one K = 6144
# block; 6121: 3072 + 3136 with 15 fillers, CRC-24B; 6200: two blocks of 3136;
# 12217: three blocks, fillers in the last size class.
CHAIN = {
    'awgn-1': (1.25, 'QPSK', 'awgn', 'siso', 1, (-5.0, 3.0), 0),
    'awgn-6120': (1.25, 'QPSK', 'awgn', 'siso', 6120, (2.5, 6.5), 0),
    'awgn-6121': (1.25, 'QPSK', 'awgn', 'siso', 6121, (2.5, 6.5), 0),
    'awgn-6200': (1.25, 'QPSK', 'awgn', 'siso', 6200, (2.5, 6.5), 0),
    'awgn-12217': (1.25, 'QPSK', 'awgn', 'siso', 12217, (2.5, 6.5), 0),
    'rayleigh-6200': (5.0, '16-QAM', 'rayleigh_mp', 'siso', 6200, (4.0, 30.0), 0),
    'sfbc-6200': (1.25, 'QPSK', 'awgn', 'sfbc', 6200, (-4.0, 1.5), 0),     # 2 RX: the cliff sits ~4 dB lower
}


SEG = {1: [(40, 15)], 6120: [(6144, 0)], 6121: [(3072, 0), (3136, 15)], 6200: [(3136, 0), (3136, 0)]}   # (K, F)


def chain_plan(C, case, prec, early_stop=True, iters=ITERS):
    import lte_phy
    bw, mod, chan, chain, n_bits, _, _ = CHAIN[case]
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=bw, modulation=mod), channel_type=chan, precision=prec)
    if chain == 'sfbc':
        return sim._sfbc_plan(0, n_bits, 2, coded=True, max_frames=FRAMES, iters=iters, early_stop=early_stop)
    return sim._plan(C.CHAIN_CODED, 0, n_bits, max_frames=FRAMES, iters=iters, early_stop=early_stop)


def chain_inputs(case):
    _, _, _, _, n_bits, (lo, hi), seed = CHAIN[case]
    bits = np.random.RandomState(chain_seed(case)).randint(0, 2, (FRAMES, n_bits)).astype(np.uint8)
    return bits, np.concatenate([np.linspace(lo, hi, 64), np.full(FRAMES - 64, hi + 6.0)])


def chain_seed(case):
    """Seed of the case's payloads and of its runs' Philox noise."""
    return CHAIN[case][4] + 100000 * CHAIN[case][6]


def chain_llrs(O, plan, case, r, b):
    """Frame b's LLRs in coded-bit order: the capture is in grid order, the T/F
    interleaver's (core/ofdm_core.py:1040-1060) with as many columns as an OFDM
    symbol carries QAM symbols (Nd, or Nd & ~1 under SFBC)."""
    bw, mod, _, chain, _, _, _ = CHAIN[case]
    bps = O.Numerology(bandwidth=bw, modulation=mod).bps
    coded, cols = plan.coded_bits, plan.res
    ncs = coded // bps
    rows = -(-ncs // cols)
    q = np.arange(ncs)
    L = r['llr'][b].astype(np.float64)
    return L.reshape(-1, bps)[(q % cols) * rows + q // cols].reshape(-1)[:coded]


def chain_reference(O, seg, L, f32, iters=ITERS, fixed=False):
    """Rate dematch, the rule per code block (or the fixed `iters` decode),
    desegmentation, the TB's CRC-24A: (bits, crc ok, n* per block, passed per block)."""
    poly = POLYS['24A'] if len(seg) == 1 else POLYS['24B']
    off, dec, ns, ps = 0, [], [], []
    for K, F, info, o, crc in seg:
        dm = O.rate_dematch(L[off:off + 3 * K + 12], K, 0)
        off += 3 * K + 12
        if f32:
            dm = dm.astype(np.float32)
        if fixed:
            d, n, p = (O.turbo_decode_f32_model if f32 else O.turbo_decode)(dm, K, iters), iters, True
        else:
            d, n, p = rule(O, dm, K, iters, poly, f32)
        dec.append(d)
        ns.append(n)
        ps.append(p)
    tbc = O.desegment(dec, seg)
    return tbc[:-24], O.check_crc24a(tbc), ns, ps


CHAIN_CASES = [(c, p) for c in CHAIN for p in ('f64', 'f32')
               if p == 'f64' or c in ('awgn-1', 'awgn-6120', 'awgn-6200', 'awgn-12217')]


@pytest.mark.parametrize('case,prec', CHAIN_CASES)
def test_chain_follows_the_rule(C, oracle, case, prec):
    O = oracle
    n_bits = CHAIN[case][4]
    plan = chain_plan(C, case, prec)
    seg = O.segmentation_plan(n_bits + 24)
    assert plan.n_cb == len(seg) and plan.coded_bits == sum(3 * s[0] + 12 for s in seg)
    if n_bits in SEG:
        assert [(s[0], s[1]) for s in seg] == SEG[n_bits]
    bits, snrs = chain_inputs(case)
    r = plan.run(snrs, seed=chain_seed(case), bits=bits, capture=('llr', 'bits_rx'))
    assert r.path['turbo'] == 'es' and r.path['dematch'] == 'llr'
    used = r['turbo_iters_used']
    assert used.shape == (FRAMES, plan.n_cb) and used.dtype == np.uint8
    n_star, passed = [], []
    for b in range(FRAMES):
        dec, ok, ns, ps = chain_reference(O, seg, chain_llrs(O, plan, case, r, b), prec == 'f32')
        assert used[b].tolist() == ns, (case, prec, b, used[b].tolist(), ns)
        assert np.array_equal(dec, r['bits_rx'][b]), (case, prec, b, int(np.sum(dec != r['bits_rx'][b])))
        assert bool(ok) == bool(r['crc_ok'][b]), (case, prec, b)
        assert int(r['frame_errors'][b]) == int(np.sum(bits[b] != dec)), (case, prec, b)
        n_star.append(ns)
        passed.append(ps)
    n_star, passed = np.array(n_star), np.array(passed)
    for k in range(plan.n_cb):       # every code-block slot has its own two waves
        assert mixing(n_star[:, k], passed[:, k]), (case, prec, k, n_star[:, k].tolist())


# ---------------------------------------------------------------------------
# (3) off means untouched
def test_fixed_plan_is_untouched(C, oracle):
    from lte_phy import engine
    case, prec, O = 'awgn-1', 'f64', oracle
    es, fx = chain_plan(C, case, prec), chain_plan(C, case, prec, early_stop=False)
    assert es is not fx and es.early_stop and not fx.early_stop
    kw = dict(N=128, Nc=72, cp_len=9, bps=2, n_sym=0, chain=C.CHAIN_CODED, channel=C.CH_AWGN, fs=1.92e6, n_bits=40,
              max_frames=4)
    assert engine.get_plan(early_stop=True, **kw) is not engine.get_plan(**kw)
    assert engine.get_plan(**kw) is engine.get_plan(early_stop=False, **kw)
    assert C.load().lte_plan_early_stop(es.h) == 1 and C.load().lte_plan_early_stop(fx.h) == 0
    bits, snrs = chain_inputs(case)
    kw = dict(seed=chain_seed(case), bits=bits, capture=('llr', 'bits_rx'))
    r = fx.run(snrs, **kw)
    assert 'turbo_iters_used' not in r and 'turbo' not in r.path
    assert set(r) == set(es.run(snrs, **kw)) - {'turbo_iters_used'}
    assert engine.path_diff(r.path, es.path(snrs, **kw)) == {'turbo'}
    out = np.zeros(FRAMES * fx.n_cb, dtype=np.uint8)
    assert C.load().lte_plan_turbo_iters_used(fx.h, C.ptr(out, C.U8), out.size) == C.LTE_EINVAL
    seg = O.segmentation_plan(CHAIN[case][4] + 24)
    differs = 0
    for b in range(FRAMES):
        L = chain_llrs(O, fx, case, r, b)
        dec, ok, _, _ = chain_reference(O, seg, L, False, fixed=True)
        assert np.array_equal(dec, r['bits_rx'][b]) and bool(ok) == bool(r['crc_ok'][b]), b
        differs += not np.array_equal(dec, chain_reference(O, seg, L, False)[0])
    assert differs > 0      # the rule's output is not the fixed decode's on these very frames


def test_iters_used_readout_checks_its_size(C):
    plan = chain_plan(C, 'awgn-1', 'f64')
    lib = C.load()
    out = np.zeros(FRAMES + 1, dtype=np.uint8)
    assert lib.lte_plan_set_early_stop(plan.h, 1) == C.LTE_OK       # setting it again forgets the last run
    assert lib.lte_plan_turbo_iters_used(plan.h, C.ptr(out, C.U8), FRAMES) == C.LTE_EINVAL
    bits, snrs = chain_inputs('awgn-1')
    plan.run(snrs[:5], seed=1, bits=bits[:5])
    assert lib.lte_plan_turbo_iters_used(plan.h, C.ptr(out, C.U8), 4) == C.LTE_EINVAL
    assert lib.lte_plan_turbo_iters_used(plan.h, C.ptr(out, C.U8), 5) == C.LTE_OK


# ---------------------------------------------------------------------------
# (4) run_grid
GRID_SNRS = [0.0, 4.0, 12.0]
GRID_T, GRID_NB, GRID_SEED = 6, 6200, 11


def grid_sim():
    import lte_phy
    return lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn',
                                 precision='f64')


def grid_oracle_n_star(O, P, frame, snr):
    """n* of every code block of one run_grid frame (SISO, AWGN): the frame's
    Philox payload and noise through the oracle's chain, then the rule."""
    num = O.Numerology(bandwidth=1.25, modulation='QPSK')
    tx = O.coded_tx(num, P.payload_bits(GRID_SEED, frame, GRID_NB))
    draws = P.siso_draws(GRID_SEED, frame, len(tx['signal']), 0)
    rx = O.channel_transmit(num, tx['signal'], 'awgn', snr, 'Pedestrian_A', 0.0, draws[0])
    L = O.coded_rx_llrs(num, rx, len(tx['coded']), snr, 'awgn')[0]
    return chain_reference(O, tx['plan'], L, False)[2]


@pytest.mark.parametrize('mimo', [None, 'sfbc'])
def test_run_grid_histogram(C, oracle, mimo):
    from oracle import philox as P
    sim = grid_sim()
    kw = dict(seed=GRID_SEED, coded=True, n_bits=GRID_NB, frames_per_call=8, turbo_iters=ITERS, mimo=mimo,
              num_rx=2 if mimo else 1, early_stop=True)
    full = sim.run_grid(GRID_SNRS, GRID_T, **kw)
    parts = [sim.run_grid(GRID_SNRS, GRID_T, rank=k, world_size=2, **kw) for k in range(2)]
    hist = full['turbo_iters_hist']
    assert hist.dtype == np.uint64 and hist.shape == (len(GRID_SNRS), ITERS + 1)
    assert np.array_equal(parts[0]['counts'] + parts[1]['counts'], full['counts'])
    assert np.array_equal(parts[0]['turbo_iters_hist'] + parts[1]['turbo_iters_hist'], hist)
    n_cb = full['plan'].n_cb
    assert n_cb == 2 and np.array_equal(hist.sum(axis=1), full['counts'][:, 3] * n_cb)
    assert np.array_equal(full['counts'][:, 3], np.full(len(GRID_SNRS), GRID_T))
    assert np.allclose(full['turbo_iters_mean'], (hist * np.arange(ITERS + 1)).sum(axis=1) / (GRID_T * n_cb))
    assert not hist[:, 0].any()
    if mimo is None:
        # the oracle's n* of the same frames: at the top SNR every block stops
        # early, at the bottom none passes -- only then the histogram's shape
        # says anything
        top, bottom = len(GRID_SNRS) - 1, 0
        want = np.zeros_like(hist)
        for s in (top, bottom):
            for t in range(GRID_T):
                for n in grid_oracle_n_star(oracle, P, s * GRID_T + t, GRID_SNRS[s]):
                    want[s, n] += 1
        assert want[top, :ITERS].sum() == GRID_T * n_cb and want[bottom, ITERS] == GRID_T * n_cb
        assert np.array_equal(hist[[top, bottom]], want[[top, bottom]])
    assert hist[-1, :ITERS].sum() == GRID_T * n_cb and full['turbo_iters_mean'][-1] < ITERS
    assert 'turbo_iters_hist' not in sim.run_grid(GRID_SNRS[-1:], 2, **dict(kw, early_stop=False))


# ---------------------------------------------------------------------------
# (5) refusals
def test_exact_logmap_refuses_early_stop(C, cc, oracle):
    plan = chain_plan(C, 'awgn-1', 'f64')
    bits, snrs = chain_inputs('awgn-1')
    llr = stage_pool(oracle, 40, '24A', False)[0]
    try:
        cc.set_decoder_mode(False)
        with pytest.raises(NotImplementedError, match='max-log'):       # LTE_EUNSUP (_capi.check)
            plan.run(snrs, seed=1, bits=bits)
        with pytest.raises(NotImplementedError, match='max-log'):
            cc.turbo_decode_early_stop(llr, 40, ITERS, '24A')
        used = np.zeros(1, dtype=np.uint8)
        out = np.zeros(40, dtype=np.uint8)
        assert C.load().lte_turbo_decode_es_host64(40, ITERS, 1, C.ptr(llr, C.F64), POLYS['24A'], C.ptr(out, C.U8),
                                                   C.ptr(used, C.U8)) == C.LTE_EUNSUP
    finally:
        cc.set_decoder_mode(True)
    assert 'turbo_iters_used' in plan.run(snrs, seed=1, bits=bits)      # and runs again in max-log mode


def test_uncoded_plans_refuse_the_switch(C):
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    plan = sim._plan(C.CHAIN_UNCODED, 14, 14 * sim.Nd * 2, max_frames=4)
    assert C.load().lte_plan_set_early_stop(plan.h, 1) == C.LTE_EINVAL
    assert C.load().lte_plan_early_stop(plan.h) == 0
    with pytest.raises(ValueError):
        sim._plan(C.CHAIN_UNCODED, 14, 14 * sim.Nd * 2, max_frames=4, early_stop=True)
    with pytest.raises(ValueError, match='early_stop'):
        sim.run_grid([10.0], 2, early_stop=True)
