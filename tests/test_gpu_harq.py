"""GPU: HARQ retransmissions with soft combining on the coded SISO chain, against
the model of tests/harq_model.py (the oracle's primitives and the bookkeeping).

  1 every round of a 4-transmission process, frame by frame: transmitted
    symbols, the model's decode of the run's own combined LLRs, the latched
    verdicts, tx_used, counts and the decoder groups skipped
  2 the same process on the symbol hand-off (k_dematch_zn adds as k_dematch)
  3 full, mixed, never-finished and partial decoder groups with LTE_HARQ_SKIP 1 / 0
  4 max_tx = 1, coded_bits = 0 is a plain coded plan, bit for bit
  5 a second process on the same plan starts clean; the round checks
  6 Philox rounds against the oracle's whole front end on seed_t's draws
  7 run_harq_grid's tables and sharding

Ladders: 67 frames (one full 64-frame decoder group and a partial one), 2
iterations, rv order (0, 2, 3, 1), SNRs linspace over the frames.  Everything is
exact except tx_syms in float32 (1e-6, as tests/test_gpu_code_blocks.py)."""
import numpy as np
import pytest

import harq_model as M

pytestmark = pytest.mark.gpu

FRAMES = 64 + 3
ITERS = 2
RV = (0, 2, 3, 1)
MAX_TX = 4
NUMS = {'A': dict(bw=1.25, mod='QPSK', chan='awgn'), 'B': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp')}
SWITCHES = ('LTE_TXCH_FUSE', 'LTE_RX_FUSE', 'LTE_TX_FRAME', 'LTE_RX_WAVE', 'LTE_TX_WAVE', 'LTE_DEMAP_IN_DEMATCH',
            'LTE_TXW_STAGE', 'LTE_TX_STAGE', 'LTE_HARQ_SKIP')
MIN_CLASS = 3
# (numerology, TB, coded_bits) -> SNR range of the 67 frames and the histogram
# [never, acknowledged after 1, 2, 3, 4 transmissions] the model gives on the
# float64 run's LLRs there.  At coded_bits = 0 every class holds at least
# MIN_CLASS frames; at the punctured budget (about 0.45 of sum(3K + 18), gamma
# != 0 in the multi-block cases) class 1 is empty by construction -- the
# window at rv 0 carries under half the systematic bits -- and the others hold
# at least MIN_CLASS.  TB 6121 at QPSK runs at 8600 bits (G' = 4300: the even
# split, gamma = 0) and at 8602 (gamma = 1: E = 4300, 4302).
LADDER = {
    ('A', 435, 0): ((-4.5, 3.5), [37, 7, 11, 8, 4]),
    ('A', 6121, 0): ((0.0, 5.0), [15, 12, 19, 17, 4]),
    ('B', 2041, 0): ((4.0, 12.0), [9, 9, 33, 8, 8]),
    ('B', 12217, 0): ((4.0, 13.5), [11, 13, 28, 7, 8]),
    ('A', 435, 640): ((1.0, 5.0), [11, 0, 18, 12, 26]),
    ('A', 6121, 8600): ((2.0, 7.5), [14, 0, 10, 11, 32]),
    ('A', 6121, 8602): ((2.0, 7.5), [14, 0, 10, 11, 32]),
    ('B', 2041, 2880): ((8.0, 15.0), [14, 0, 12, 13, 28]),
    ('B', 12217, 17000): ((6.5, 21.5), [15, 0, 28, 9, 15]),
}
CASES = list(LADDER)


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


def clear_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def make_plan(C, O, name, n_bits, prec, harq, frames=FRAMES, iters=ITERS):
    import lte_phy
    nm = NUMS[name]
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=nm['bw'], modulation=nm['mod']),
                                channel_type=nm['chan'], precision=prec)
    plan = sim._plan(C.CHAIN_CODED, 0, n_bits, max_frames=frames, iters=iters, harq=harq)
    num = O.Numerology(bandwidth=nm['bw'], modulation=nm['mod'])
    assert plan.Nd == num.Nd
    return plan, num


def ladder_inputs(case):
    name, n_bits, G = case
    bits = np.random.RandomState(n_bits).randint(0, 2, (FRAMES, n_bits)).astype(np.uint8)
    lo, hi = LADDER[case][0]
    return bits, np.linspace(lo, hi, FRAMES)


def harq_plan(C, O, case, prec):
    name, n_bits, G = case
    plan, num = make_plan(C, O, name, n_bits, prec, dict(max_tx=MAX_TX, rv_seq=RV, coded_bits=G))
    Ks, Es = M.split(O, n_bits, num.bps, G)
    info = plan.harq_info()
    assert (info['max_tx'], info['n_cb'], info['E'], info['coded_bits']) == (MAX_TX, len(Ks), Es, sum(Es))
    assert plan.coded_bits == sum(Es) and plan.n_sym == -(-(-(-sum(Es) // num.bps)) // num.Nd)
    if G and len(Ks) > 1 and G != 8600:
        assert (G // num.bps) % len(Ks) != 0 and len(set(Es)) == 2        # gamma != 0
    return plan, num, Es


def check_counts(r, proc, tag):
    assert np.array_equal(r['counts'], proc.counts()), (tag, r['counts'], proc.counts())


# ---------------------------------------------------------------------------
# 1 round-by-round exactness
CAP1 = ('tx_syms', 'llr', 'bits_rx')


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s-%d-%d' % c)
def test_rounds_equal_the_model(C, oracle, monkeypatch, case, prec):
    """Injected bits, the device's own noise, LLRs captured, the rounds driven
    one by one.  Per round and frame: tx_syms are the model's QAM of
    rate_match(., E_r, K_r, rv_t); the model adds the run's own LLRs to its
    sums (float32 sums in f32) and decodes them -> bits_rx; the latched crc_ok /
    frame_errors / tx_used, counts and the number of finished groups the
    decoder skipped equal the model's.  Then the sensitivity condition: the
    frames fall into every acknowledgement class (LADDER)."""
    clear_switches(monkeypatch)
    O = oracle
    name, n_bits, G = case
    plan, num, Es = harq_plan(C, O, case, prec)
    bits, snrs = ladder_inputs(case)
    tag = '%s/%d/%d/%s' % (name, n_bits, G, prec)
    enc = [M.encode(O, bits[b]) for b in range(FRAMES)]
    seg = enc[0][1]
    proc = M.Process(O, seg, Es, RV, bits, ITERS, f32=(prec == 'f32'))
    for t in range(MAX_TX):
        plan.harq_round(t)
        r = plan.run(snrs, seed=n_bits, bits=bits, capture=CAP1)
        assert r.path['dematch'] == 'llr' and r.path['harq'] == 't%d,rv%d,skip=%d' % (t, RV[t], t > 0), r.path
        for b in range(FRAMES):
            qam, pos = M.tx_qam(O, num, enc[b][0], seg, Es, RV[t])
            ts = r['tx_syms'][b].astype(np.complex128)[pos]
            if prec == 'f64':
                assert np.array_equal(ts, qam), (tag, t, b)
            else:
                assert np.max(np.abs(ts - qam)) < 1e-6, (tag, t, b)
        llr = [M.llr_coded_order(r['llr'][b], num, sum(Es)) for b in range(FRAMES)]
        m = proc.round(t, llr)
        for k in ('bits_rx', 'crc_ok', 'frame_errors', 'tx_used'):
            bad = np.flatnonzero(np.any(np.atleast_2d(r[k].T != m[k].T), axis=0))
            assert np.array_equal(r[k], m[k]), (tag, t, k, bad)
        assert r['harq_info']['round'] == t and r['harq_info']['rv'] == RV[t]
        assert r['harq_info']['skipped'] == m['skipped'], (tag, t)
        check_counts(r, proc, (tag, t))
    hist = M.histogram(m['tx_used'], m['crc_ok'], MAX_TX)
    print('histogram', tag, hist)
    need = [0, 1, 2, 3, 4] if G == 0 else [0, 2, 3, 4]
    assert all(hist[c] >= MIN_CLASS for c in need), (tag, hist)
    if G:
        assert hist[1] == 0, (tag, hist)
    if prec == 'f64' and LADDER[case][1] is not None:
        assert hist == LADDER[case][1], (tag, hist)


# ---------------------------------------------------------------------------
# 2 fused path
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s-%d-%d' % c)
def test_rounds_on_the_symbol_handoff(C, oracle, monkeypatch, case, prec):
    """The same process without the LLR capture (16-QAM demaps inside
    k_dematch_zn, which adds to the rows as k_dematch does): identical latched
    results and decisions, round by round; the paths differ in dematch / rx only."""
    from lte_phy.engine import path_diff
    clear_switches(monkeypatch)
    name, n_bits, G = case
    plan, num, Es = harq_plan(C, oracle, case, prec)
    bits, snrs = ladder_inputs(case)
    keys = ('bits_rx', 'crc_ok', 'frame_errors', 'tx_used', 'counts')
    runs = {}
    for cap in (CAP1, ('bits_rx',)):
        for t in range(MAX_TX):
            plan.harq_round(t)
            r = plan.run(snrs, seed=n_bits, bits=bits, capture=cap)
            runs[len(cap), t] = (r.path, {k: r[k].copy() for k in keys}, r['harq_info']['skipped'])
    for t in range(MAX_TX):
        (p1, r1, s1), (p2, r2, s2) = runs[3, t], runs[1, t]
        assert p1['dematch'] == 'llr' and p2['dematch'] == ('zn' if num.bps > 2 else 'llr')
        assert path_diff(p1, p2) <= {'dematch', 'rx'}, (p1, p2)
        assert s1 == s2
        for k in keys:
            assert np.array_equal(r1[k], r2[k]), (case, prec, t, k)
    assert 0 < int(np.sum(runs[1, MAX_TX - 1][1]['crc_ok'])) < FRAMES


# ---------------------------------------------------------------------------
# 3 groups and the skip
HI_DB, LO_DB = 12.0, -20.0     # numerology A, TB 435, 3K + 12 bits per transmission: every frame passes at
#                                once / no frame passes in four transmissions (asserted on the model)


def group_snrs():
    lo, hi = LADDER['A', 435, 0][0]
    return np.concatenate([np.full(64, HI_DB), np.linspace(lo, hi, 64), np.full(64, LO_DB), np.linspace(lo, hi, 5)])


def test_groups_and_the_skip(C, oracle, monkeypatch):
    """197 frames: a group finished in round 0, a ladder group, a group that
    never finishes and a 5-frame partial group.  Plan.run_harq with
    LTE_HARQ_SKIP 1 and 0: identical latched results and counts per round, equal
    to the model; with the skip on, each round reports exactly the groups the
    model had finished before it, and the path names the decoder family."""
    clear_switches(monkeypatch)
    O = oracle
    n_bits, B = 435, 197
    plan, num = make_plan(C, O, 'A', n_bits, 'f64', dict(max_tx=MAX_TX, rv_seq=RV, coded_bits=0), frames=B)
    Ks, Es = M.split(O, n_bits, num.bps, 0)
    bits = np.random.RandomState(3).randint(0, 2, (B, n_bits)).astype(np.uint8)
    snrs = group_snrs()
    kw = dict(seed=7, bits=bits)
    monkeypatch.setenv('LTE_HARQ_SKIP', '1')
    on = plan.run_harq(snrs, capture=('llr',), **kw)
    monkeypatch.setenv('LTE_HARQ_SKIP', '0')
    off = plan.run_harq(snrs, **kw)
    assert on.path['harq'] == 't3,rv1,skip=1' and off.path['harq'] == 't3,rv1,skip=0'
    assert on['rounds_run'] == off['rounds_run'] == MAX_TX
    for k in ('tx_used', 'crc_ok', 'frame_errors', 'counts_by_round'):
        assert np.array_equal(on[k], off[k]), k
    assert off['skipped'] == [0, 0, 0, 0]
    seg = O.segmentation_plan(n_bits + 24)
    proc = M.Process(O, seg, Es, RV, bits, ITERS)
    for t in range(MAX_TX):
        llr = [M.llr_coded_order(on['rounds'][t]['llr'][b], num, sum(Es)) for b in range(B)]
        m = proc.round(t, llr)
        assert on['skipped'][t] == m['skipped'], (t, on['skipped'], m['skipped'])
        assert np.array_equal(on['counts_by_round'][t], proc.counts()), t
        if t == 0:
            assert m['crc_ok'][:64].all() and m['skipped'] == 0
        else:
            assert 0 in proc.finished_groups() and m['skipped'] >= 1
    for k in ('tx_used', 'crc_ok', 'frame_errors'):
        assert np.array_equal(on[k], m[k]), k
    assert not m['crc_ok'][128:192].any() and (m['tx_used'][128:192] == MAX_TX).all()
    assert 2 not in proc.finished_groups()
    # every frame at the high SNR: one round, and nothing left to send
    monkeypatch.delenv('LTE_HARQ_SKIP')
    one = plan.run_harq(np.full(B, HI_DB), **kw)
    assert one['rounds_run'] == 1 and one['crc_ok'].all() and (one['tx_used'] == 1).all()
    assert np.array_equal(one['counts_by_round'], np.repeat(one['counts'][None], MAX_TX, axis=0))


def test_all_groups_finished_launches_no_decoder(C, oracle, monkeypatch):
    """A round driven by hand after every frame is acknowledged: all groups are
    skipped, the turbo timer sees no launch, the results stay latched."""
    clear_switches(monkeypatch)
    n_bits, B = 435, 70
    plan, num = make_plan(C, oracle, 'A', n_bits, 'f64', dict(max_tx=2, rv_seq=RV, coded_bits=0), frames=FRAMES + 3)
    kw = dict(seed=9)
    plan.harq_round(0)
    r0 = plan.run(np.full(B, HI_DB), capture=('bits_rx',), **kw)
    assert r0['crc_ok'].all()
    plan.timing(True)
    plan.timing_reset()
    plan.harq_round(1)
    r1 = plan.run(np.full(B, LO_DB), capture=('bits_rx',), **kw)
    plan.timing(False)
    tim = plan.timing_read()
    assert tim['turbo'][1] == 0 and tim['harq'][1] == 1 and tim['crc_count'][1] == 1, tim
    assert r1['harq_info']['skipped'] == 2
    for k in ('crc_ok', 'frame_errors', 'tx_used', 'bits_rx', 'counts'):
        assert np.array_equal(r0[k], r1[k]), k


# ---------------------------------------------------------------------------
# 4 identity with the plain chain
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name,n_bits,snr', [('A', 435, (-2.0, 10.0)), ('B', 2041, (0.0, 30.0)),
                                            ('B', 12217, (0.0, 30.0))])
def test_one_transmission_is_the_plain_chain(C, oracle, monkeypatch, name, n_bits, snr, prec):
    clear_switches(monkeypatch)
    hq, _ = make_plan(C, oracle, name, n_bits, prec, dict(max_tx=1, rv_seq=(0,), coded_bits=0))
    plain, _ = make_plan(C, oracle, name, n_bits, prec, None)
    assert hq is not plain
    geo = ('L', 'n_sym', 'Nd', 'Np', 'n_grp', 'n_cb', 'coded_bits', 'n_re_bits')
    assert [getattr(hq, k) for k in geo] == [getattr(plain, k) for k in geo]
    snrs = np.linspace(snr[0], snr[1], FRAMES)
    ids = np.arange(FRAMES, dtype=np.uint64) * 3 + 11
    kw = dict(seed=2041, frame_ids=ids, capture=('bits_rx',))
    a, b = hq.run(snrs, **kw), plain.run(snrs, **kw)
    for k in ('counts', 'frame_errors', 'crc_ok', 'bits_rx'):
        assert np.array_equal(a[k], b[k]), k
    assert 0 < int(a['crc_ok'].sum()) < FRAMES
    assert 'harq' not in b.path and a.path['harq'] == 't0,rv0,skip=0'
    assert {k: v for k, v in a.path.items() if k != 'harq'} == b.path
    assert (a['tx_used'] == 1).all()


# ---------------------------------------------------------------------------
# 5 process hygiene
def test_a_new_process_starts_clean_and_rounds_are_checked(C, oracle, monkeypatch):
    """After a four-round process at the punctured budget (whose later rounds
    fill rows that round 0's window leaves out), round 0 with other bits on the
    same plan gives what a new plan gives.  Then the refusals."""
    from lte_phy import engine
    clear_switches(monkeypatch)
    case = ('B', 2041, 2880)
    name, n_bits, G = case
    plan, num, Es = harq_plan(C, oracle, case, 'f64')
    bits, snrs = ladder_inputs(case)
    first = plan.run_harq(snrs, seed=1, bits=bits)
    assert first['rounds_run'] == MAX_TX
    bits2 = np.random.RandomState(99).randint(0, 2, (FRAMES, n_bits)).astype(np.uint8)
    kw = dict(seed=5, bits=bits2, capture=('bits_rx',))
    plan.harq_round(0)
    again = plan.run(snrs, **kw)
    engine.clear_cache()
    fresh, _, _ = harq_plan(C, oracle, case, 'f64')
    assert fresh is not plan
    new = fresh.run(snrs, **kw)
    for k in ('counts', 'frame_errors', 'crc_ok', 'bits_rx', 'tx_used'):
        assert np.array_equal(again[k], new[k]), k
    assert (again['tx_used'] == 1).all()
    # lte_run without set_round is round 0 again
    assert plan.run(snrs, **kw).path['harq'].startswith('t0,')
    lib = C.load()
    with pytest.raises(ValueError, match='HARQ'):
        plan.harq_round(2)                               # round 1 has not run
    plan.harq_round(1)
    with pytest.raises(ValueError, match='n_frames'):
        plan.run(snrs[:-1], seed=5, bits=bits2[:-1])
    plan.harq_round(1)
    with pytest.raises(ValueError, match='frame ids'):
        plan.run(snrs, seed=5, bits=bits2, frame_id0=1)
    with pytest.raises(ValueError, match='max_tx'):
        plan.harq_round(MAX_TX)
    assert lib.lte_plan_harq_set_round(plan.h, -1) == C.LTE_EINVAL
    assert lib.lte_plan_set_early_stop(plan.h, 1) == C.LTE_EUNSUP
    assert b'HARQ' in lib.lte_last_error()
    # the process is still where it was: round 1 with round 0's frames runs
    plan.harq_round(1)
    r1 = plan.run(snrs, seed=5, bits=bits2)
    assert r1['harq_info']['round'] == 1 and (r1['tx_used'][r1['crc_ok'] == 0] == 2).all()


def test_decoder_mode_0_runs_without_the_skip(C, oracle, monkeypatch):
    """Exact log-MAP (float64 only): the rounds run, every group is decoded."""
    from lte_phy import channel_coding as cc
    clear_switches(monkeypatch)
    plan, num = make_plan(C, oracle, 'A', 435, 'f64', dict(max_tx=2, rv_seq=RV, coded_bits=0))
    snrs = np.concatenate([np.full(64, HI_DB), np.full(3, LO_DB)])
    try:
        cc.set_decoder_mode(False)
        r = plan.run_harq(snrs, seed=4)
    finally:
        cc.set_decoder_mode(True)
    assert r['rounds_run'] == 2 and r['skipped'] == [0, 0] and r.path['harq'] == 't1,rv2,skip=0'
    assert r['crc_ok'][:64].all() and (r['tx_used'][:64] == 1).all() and (r['tx_used'][64:] == 2).all()


# ---------------------------------------------------------------------------
# 6 Philox rounds
def test_philox_rounds_match_the_oracle_front_end(C, oracle, monkeypatch):
    """Nothing injected: per frame, tx_used / crc_ok / frame_errors equal the
    model run through oracle.channel_transmit and coded_rx_llrs on
    philox.siso_draws(seed_t, id, L, 4), the payload on `seed`.  Round 1's LLRs
    differ from round 0's, and another batch order gives the same per-frame
    results."""
    from oracle import philox as P
    clear_switches(monkeypatch)
    O = oracle
    case, seed, iters = ('B', 2041, 2880), 0xC0FFEE, 2
    name, n_bits, G = case
    n = 16
    plan, num = make_plan(C, O, name, n_bits, 'f64', dict(max_tx=MAX_TX, rv_seq=RV, coded_bits=G), frames=n)
    Ks, Es = M.split(O, n_bits, num.bps, G)
    ids = (np.arange(n, dtype=np.uint64) * 4099 + 5)
    snrs = np.linspace(0.0, 34.0, n)
    bits = np.stack([P.payload_bits(seed, int(f), n_bits) for f in ids])
    enc = [M.encode(O, bits[b]) for b in range(n)]
    seg = enc[0][1]
    proc = M.Process(O, seg, Es, RV, bits, iters)
    got = plan.run_harq(snrs, seed=seed, frame_ids=ids, capture=('llr',))
    for t in range(got['rounds_run']):
        llr = []
        for b in range(n):
            qam, _ = M.tx_qam(O, num, enc[b][0], seg, Es, RV[t])
            sig = M.tx_signal(O, num, qam)
            assert len(sig) == plan.L
            d = P.siso_draws(M.seed_t(seed, t), int(ids[b]), plan.L, 4)[0]
            rx = O.channel_transmit(num, sig, 'rayleigh_mp', float(snrs[b]), 'Pedestrian_A', 0.0, d)
            llr.append(O.coded_rx_llrs(num, rx, sum(Es), float(snrs[b]), 'rayleigh_mp')[0])
        m = proc.round(t, llr)
    for k in ('tx_used', 'crc_ok', 'frame_errors'):
        assert np.array_equal(got[k], m[k]), (k, got[k], m[k])
    assert len(set(got['tx_used'].tolist())) >= 2 and 0 < int(got['crc_ok'].sum()) < n
    l0, l1 = got['rounds'][0]['llr'], got['rounds'][1]['llr']
    assert not np.array_equal(l0, l1) and np.all(np.any(l0 != l1, axis=1))
    order = np.random.RandomState(1).permutation(n)
    other = plan.run_harq(snrs[order], seed=seed, frame_ids=ids[order])
    for k in ('tx_used', 'crc_ok', 'frame_errors'):
        assert np.array_equal(other[k], got[k][order]), k


# ---------------------------------------------------------------------------
# 7 grid
def test_run_harq_grid(C, monkeypatch):
    import lte_phy
    clear_switches(monkeypatch)
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    snrs, T = [-6.0, -2.0, 3.0], 64
    kw = dict(seed=3, n_bits=435, frames_per_call=100, turbo_iters=ITERS)
    g = sim.run_harq_grid(snrs, T, **kw)
    assert g['counts_by_round'].shape == (3, MAX_TX, 4) and g['counts_by_round'].dtype == np.uint64
    assert g['tx_hist'].shape == (3, MAX_TX + 1) and np.array_equal(g['tx_hist'].sum(axis=1), [T] * 3)
    assert np.array_equal(g['counts_by_round'][:, :, 3], np.full((3, MAX_TX), T))
    bler = g['counts_by_round'][:, :, 2] / T
    assert np.array_equal(g['bler_by_tx'], bler) and np.all(np.diff(bler, axis=1) <= 0)
    # acknowledged after at most t + 1 transmissions = the blocks round t no longer counts as errors
    assert np.array_equal(np.cumsum(g['tx_hist'][:, 1:], axis=1), T - g['counts_by_round'][:, :, 2])
    sent = (g['tx_hist'][:, 1:] * np.arange(1, MAX_TX + 1)).sum(axis=1) + MAX_TX * g['tx_hist'][:, 0]
    assert np.allclose(g['mean_tx'], sent / T)
    assert np.allclose(g['throughput'], 435 * g['tx_hist'][:, 1:].sum(axis=1) / sent)
    assert g['code_rate'] == (435 + 24) / (3 * 464 + 12)
    assert g['bler_by_tx'][0, 0] > g['bler_by_tx'][2, 0] and g['mean_tx'][0] > g['mean_tx'][2]
    parts = [sim.run_harq_grid(snrs, T, rank=r, world_size=2, **kw) for r in range(2)]
    for k in ('counts_by_round', 'tx_hist'):
        assert np.array_equal(parts[0][k] + parts[1][k], g[k]), k
