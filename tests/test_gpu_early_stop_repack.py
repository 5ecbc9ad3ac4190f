"""GPU: re-packing of the early-stop decoders' undecided blocks (k_turbo64_esw /
k_turbo_esw, k_repack_index / _gather / _scatter).

The contract: with a boundary `after`, every output is bit for bit that of the
same early-stop decode without re-packing, which tests/test_gpu_early_stop.py
ties to the rule (n* = the first iteration whose decisions pass the CRC-24).
What re-packing changes is reported by its info: the blocks undecided at the
boundary (n* > after), the 64-block groups that ran the remaining iterations,
and whether they were packed, continued in place, or nothing was left.

  (1) the stage entries against the rule: four waves with stragglers that fit
      one packed group, a wave of decided blocks, a partial wave
  (2) counts at the edges: none, all, 64, 65, the capacity and one more
  (3) the coded chains against the same plan without re-packing, 259 frames
  (4) source rows chunked by 32 with plain packed rows, and both chunked
  (5) the other coded chains through run_grid / run_scfdm_grid
  (6) switching on and off, refusals   (7) device memory
Every comparison is exact."""
import numpy as np
import pytest

from test_gpu_early_stop import CHAIN, ITERS, POLYS, chain_llrs, chain_reference, chain_seed, rule

pytestmark = pytest.mark.gpu


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
# (1) stage entries
# K -> (ladder of per-block SNRs in dB, seed per generator).  The seeds were
# moved (never the condition of `kinds`) until each pool offers, for after = 1,
# 2 and 7 alike, blocks decided by `after`, blocks decided later (for after = 7:
# one that passes at the eighth iteration exactly) and blocks that never pass.
STAGE = {40: (np.linspace(0.0, 4.0, 47), {'24A': 61, '24B': 33}), 56: (np.linspace(0.0, 4.0, 47), {'24A': 8, '24B': 42}),
         64: (np.linspace(0.0, 4.0, 47), {'24A': 72, '24B': 3}), 1056: (np.linspace(2.6, 3.6, 15), {'24A': 50, '24B': 95})}
AFTERS = [1, 2, 7]
_POOL = {}


def stage_pool(O, K, crc, f32, iters=ITERS):
    """Blocks of one K as tests/test_gpu_early_stop.py draws them (payload +
    CRC-24, turbo-encoded, BPSK LLRs at the block's own SNR, last the all-zero
    word): (llr [n][3K+12], D(n*), n*, passed), the rule by the oracle."""
    key = (K, crc, f32, iters)
    if key not in _POOL:
        snrs, seeds = STAGE[K]
        rs = np.random.RandomState(1000 * seeds[crc] + K)
        llr = []
        for snr in snrs:
            p = rs.randint(0, 2, K - 24).astype(np.uint8)
            cb = np.concatenate([p, O.crc_bits(p, POLYS[crc], 24)])
            s2 = 10 ** (-snr / 10)
            y = 1 - 2.0 * O.turbo_encode(cb) + np.sqrt(s2) * rs.randn(3 * K + 12)
            llr.append(2 * y / s2)
        llr.append(np.full(3 * K + 12, 8.0))
        llr = np.array(llr, dtype=np.float32 if f32 else np.float64)
        res = [rule(O, l, K, iters, POLYS[crc], f32) for l in llr]
        _POOL[key] = (llr, np.array([r[0] for r in res]), np.array([r[1] for r in res]),
                      np.array([r[2] for r in res]))
    return _POOL[key]


def kinds(n_star, passed, after):
    """Pool indices by kind at the boundary: decided by `after`, decided later, never passing."""
    return (np.flatnonzero(passed & (n_star <= after)), np.flatnonzero(passed & (n_star > after)),
            np.flatnonzero(~passed))


def take(idx, n, start=0):
    return idx[(start + np.arange(n)) % len(idx)]


def stage_lanes(n_star, passed, after):
    """323 lanes: waves 0..3 hold 60 blocks decided by `after`, three decided
    later and one that never passes (at places that differ from wave to wave);
    wave 4 and the three lanes of wave 5 hold decided blocks only."""
    dec, late, never = kinds(n_star, passed, after)
    waves = []
    for w in range(4):
        lanes = np.concatenate([take(late, 3, 3 * w), take(never, 1, w), take(dec, 60, 60 * w)])
        waves.append(np.roll(lanes, 1 + 17 * w))
    return np.concatenate(waves + [take(dec, 64, 7), take(dec, 3, 11)])


@pytest.mark.parametrize('after', AFTERS)
@pytest.mark.parametrize('crc', ['24A', '24B'])
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('K', sorted(STAGE))
def test_stage_entry_follows_the_rule(cc, oracle, K, prec, crc, after):
    f32 = prec == 'f32'
    llr, d, n_star, passed = stage_pool(oracle, K, crc, f32)
    dec, late, never = kinds(n_star, passed, after)
    assert len(dec) and len(late) and len(never), (K, prec, crc, after, n_star.tolist(), passed.tolist())
    lanes = stage_lanes(n_star, passed, after)
    und = n_star[lanes] > after
    assert len(lanes) == 323 and und.sum() == 16 and all(und[64 * w:64 * w + 64].sum() == 4 for w in range(4))
    bits, used, info = cc.turbo_decode_early_stop(llr[lanes], K, ITERS, crc, precision=prec, repack=after)
    assert used.dtype == np.uint8 and bits.shape == (len(lanes), K)
    assert np.array_equal(used, n_star[lanes]), (K, prec, crc, after, used.tolist(), n_star[lanes].tolist())
    assert np.array_equal(bits, d[lanes]), (K, prec, crc, after, np.flatnonzero((bits != d[lanes]).any(axis=1)).tolist())
    assert info == {'undecided': 16, 'groups': 1, 'state': 'packed'}, info


# ---------------------------------------------------------------------------
# (2) counts at the edges (K = 40, gCRC24B pool)
def edge_lanes(n_star, passed, after, n, n_und, seed):
    """n lanes of which n_und are undecided at the boundary (later-deciding and
    never-passing blocks alternating), at random places."""
    dec, late, never = kinds(n_star, passed, after)
    und = np.concatenate([take(late, n_und), take(never, n_und)]).reshape(2, -1).T.ravel()[:n_und]
    lanes = np.concatenate([und, take(dec, n - n_und)]).astype(np.int64)
    return lanes[np.random.RandomState(seed).permutation(n)]


# 323 blocks: 6 groups, so the packed arrays hold max(1, ceil(6 / 4)) = 2 groups = 128 blocks
EDGES = {'none': (323, 0, 0, 'none'), 'all': (131, 131, 3, 'in_place'), '64': (323, 64, 1, 'packed'),
         '65': (323, 65, 2, 'packed'), 'capacity': (323, 128, 2, 'packed'), 'capacity+1': (323, 129, 6, 'in_place'),
         'one-block': (1, 1, 1, 'in_place'), 'one-of-two': (2, 1, 1, 'packed')}


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('edge', sorted(EDGES))
def test_stage_entry_counts_at_the_edges(cc, oracle, edge, prec):
    n, n_und, groups, state = EDGES[edge]
    llr, d, n_star, passed = stage_pool(oracle, 40, '24B', prec == 'f32')
    lanes = edge_lanes(n_star, passed, 1, n, n_und, seed=n_und)
    if edge == 'all':
        lanes = take(kinds(n_star, passed, 1)[2], n)             # blocks that never pass only
    assert (n_star[lanes] > 1).sum() == n_und
    bits, used, info = cc.turbo_decode_early_stop(llr[lanes], 40, ITERS, '24B', precision=prec, repack=1)
    assert np.array_equal(used, n_star[lanes]) and np.array_equal(bits, d[lanes]), (edge, prec)
    assert info == {'undecided': n_und, 'groups': groups, 'state': state}, (edge, info)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_stage_entry_two_iterations(cc, oracle, prec):
    """turbo_iters 2 with the boundary at 1: the second window is the decoder-2
    pass of the first iteration and the final pass."""
    llr, d, n_star, passed = stage_pool(oracle, 40, '24B', prec == 'f32', iters=2)
    assert set(n_star.tolist()) == {1, 2} and not passed.all()
    lanes = np.arange(131) % len(llr)
    bits, used, info = cc.turbo_decode_early_stop(llr[lanes], 40, 2, '24B', precision=prec, repack=1)
    assert np.array_equal(used, n_star[lanes]) and np.array_equal(bits, d[lanes])
    n_und = int((n_star[lanes] > 1).sum())
    assert 0 < n_und < 131
    # three groups, so one packed group: packed if the undecided blocks fit it, else in place
    want = {'undecided': n_und, 'groups': 1, 'state': 'packed'} if n_und <= 64 else \
        {'undecided': n_und, 'groups': 3, 'state': 'in_place'}
    assert info == want, info


def test_stage_entry_second_call_on_fewer_blocks(cc, oracle):
    llr, d, n_star, passed = stage_pool(oracle, 40, '24B', False)
    big = edge_lanes(n_star, passed, 1, 323, 100, seed=5)
    cc.turbo_decode_early_stop(llr[big], 40, ITERS, '24B', repack=1)
    small = edge_lanes(n_star, passed, 1, 70, 3, seed=6)
    bits, used, info = cc.turbo_decode_early_stop(llr[small], 40, ITERS, '24B', repack=1)
    assert np.array_equal(used, n_star[small]) and np.array_equal(bits, d[small])
    assert info == {'undecided': 3, 'groups': 1, 'state': 'packed'}, info


# ---------------------------------------------------------------------------
# (3) the coded chains: 259 frames = five groups per code-block slot, capacity two
FRAMES = 259
CAP = 2
AFTER = 1
RP_CASES = [(c, p) for c in ('awgn-1', 'awgn-6121', 'awgn-12217', 'rayleigh-6200', 'sfbc-6200') for p in ('f64', 'f32')
            if p == 'f64' or c.startswith('awgn')]
RULE_CASES = {('awgn-1', 'f64'), ('awgn-6121', 'f64')}      # also against the oracle's rule, frames 0..66


def rp_plan(C, case, prec, repack, max_frames=FRAMES):
    import lte_phy
    bw, mod, chan, chain, n_bits, _, _ = CHAIN[case]
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=bw, modulation=mod), channel_type=chan, precision=prec)
    if chain == 'sfbc':
        return sim._sfbc_plan(0, n_bits, 2, coded=True, max_frames=max_frames, iters=ITERS, early_stop=True,
                              repack=repack)
    return sim._plan(C.CHAIN_CODED, 0, n_bits, max_frames=max_frames, iters=ITERS, early_stop=True, repack=repack)


def rp_inputs(case):
    """Frames 0..63 on the case's own ladder; of the rest most 6 dB above it
    (decided at once) and the last 24 on the ladder again, so every slot keeps
    undecided blocks in several groups and they fit the two packed groups."""
    _, _, _, _, n_bits, (lo, hi), _ = CHAIN[case]
    bits = np.random.RandomState(chain_seed(case) + 1).randint(0, 2, (FRAMES, n_bits)).astype(np.uint8)
    snrs = np.concatenate([np.linspace(lo, hi, 64), np.full(FRAMES - 64 - 24, hi + 6.0), np.linspace(lo, hi, 24)])
    return bits, snrs


def expected_info(used, after, cap):
    """repack_info as the plain run's own n* imply it."""
    und = [int(v) for v in (used > after).sum(axis=0)]
    B = used.shape[0]
    state = ['none' if u == 0 else 'packed' if u <= 64 * cap and u < B else 'in_place' for u in und]
    groups = [0 if s == 'none' else -(-u // 64) if s == 'packed' else -(-B // 64) for u, s in zip(und, state)]
    return {'after': after, 'n_cb': used.shape[1], 'undecided': und, 'groups': groups, 'state': state}


SAME = ('turbo_iters_used', 'bits_rx', 'crc_ok', 'frame_errors', 'counts')


@pytest.mark.parametrize('case,prec', RP_CASES)
def test_chain_equals_plain_early_stop(C, oracle, case, prec):
    plain, rp = rp_plan(C, case, prec, None), rp_plan(C, case, prec, AFTER)
    assert plain is not rp and plain.repack == 0 and rp.repack == AFTER
    assert C.load().lte_plan_early_stop_repack(rp.h) == AFTER and C.load().lte_plan_early_stop(rp.h) == 1
    bits, snrs = rp_inputs(case)
    kw = dict(seed=chain_seed(case), bits=bits, capture=('llr', 'bits_rx'))
    a, b = plain.run(snrs, **kw), rp.run(snrs, **kw)
    used = a['turbo_iters_used']
    und = (used > AFTER).sum(axis=0)
    assert (und > 0).all() and (und <= 64 * CAP).all(), (case, prec, und.tolist())    # the ladder's own condition
    for k in SAME:
        assert np.array_equal(a[k], b[k]), (case, prec, k)
    assert 'repack_info' not in a and b['repack_info'] == expected_info(used, AFTER, CAP), (case, b['repack_info'])
    assert b['repack_info']['state'] == ['packed'] * rp.n_cb
    assert b.path['turbo'] == 'es' and b.path['repack'] == str(AFTER) and 'repack' not in a.path
    # a second run on fewer frames: nothing of the first is left over
    a2, b2 = plain.run(snrs[:67], **dict(kw, bits=bits[:67])), rp.run(snrs[:67], **dict(kw, bits=bits[:67]))
    for k in SAME:
        assert np.array_equal(a2[k], b2[k]), (case, prec, k)
    assert b2['repack_info'] == expected_info(a2['turbo_iters_used'], AFTER, CAP)
    if (case, prec) in RULE_CASES:
        O = oracle
        seg = O.segmentation_plan(CHAIN[case][4] + 24)
        for f in range(67):
            dec, ok, ns, _ = chain_reference(O, seg, chain_llrs(O, rp, case, b, f), prec == 'f32')
            assert b['turbo_iters_used'][f].tolist() == ns, (case, f)
            assert np.array_equal(dec, b['bits_rx'][f]) and bool(ok) == bool(b['crc_ok'][f]), (case, f)


# ---------------------------------------------------------------------------
# (4) chunked rows: TB of 16 bits = one K = 40 block, QPSK on AWGN, Philox payloads
def small_plan(C, frames, repack, prec='f64'):
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn',
                                precision=prec)
    return sim._plan(C.CHAIN_CODED, 0, 16, max_frames=frames, iters=ITERS, early_stop=True, repack=repack)


@pytest.mark.parametrize('frames,src_chunked,packed_chunked', [(2048 + 67, True, False), (8192 + 3, True, True)])
def test_chunked_rows(C, frames, src_chunked, packed_chunked):
    G = -(-frames // 64)
    cap = max(1, -(-G // 4))
    assert (G >= 32) == src_chunked and (cap >= 32) == packed_chunked
    plain, rp = small_plan(C, frames, None), small_plan(C, frames, AFTER)
    assert plain.n_cb == 1
    # one frame in eight on the ladder over the cliff, the others well above it
    snrs = np.where(np.arange(frames) % 8 == 3, np.linspace(-5.0, 3.0, frames), 9.0)
    ids = np.arange(frames, dtype=np.uint64) + 1000
    kw = dict(seed=77, frame_ids=ids, capture=('bits_rx',))
    a, b = plain.run(snrs, **kw), rp.run(snrs, **kw)
    und = int((a['turbo_iters_used'] > AFTER).sum())
    assert 64 * (cap - 1) // 4 < und <= 64 * cap, (und, cap)     # several packed groups, within the capacity
    for k in SAME:
        assert np.array_equal(a[k], b[k]), (frames, k)
    assert b['repack_info'] == {'after': AFTER, 'n_cb': 1, 'undecided': [und], 'groups': [-(-und // 64)],
                                'state': ['packed']}


# ---------------------------------------------------------------------------
# (5) the other coded chains through the public calls
# QPSK on AWGN at 1.25 MHz, TB 435 (one code block), the SNR windows over each chain's cliff that
# tests/test_gpu_s*_coded.py use for their grids, 100 trials per point: 300 frames in calls of 160
def grid_calls():
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn',
                                precision='f64')
    common = dict(seed=21, n_bits=435, frames_per_call=160, turbo_iters=ITERS, early_stop=True)
    sp = {'num_tx': 2, 'num_rx': 2, 'rank': 2, 'detector': 'MMSE', 'pmi': 0}
    return {'simo': (lambda **k: sim.run_grid([-2.0, 1.0, 4.0], 100, coded=True, num_rx=2, **common, **k)),
            'spatial': (lambda **k: sim.run_grid([4.0, 12.0, 20.0], 100, coded=True, mimo='spatial', spatial=sp,
                                                 **common, **k)),
            'scfdm': (lambda **k: sim.run_scfdm_grid([0.0, 3.0, 6.0], 100, **common, **k))}


@pytest.mark.parametrize('chain', ['simo', 'spatial', 'scfdm'])
def test_grid_drivers(chain):
    call = grid_calls()[chain]
    plain, rp = call(), call(repack=1)
    assert rp['plan'] is not plain['plan'] and rp['plan'].repack == 1 and plain['plan'].repack == 0
    assert np.array_equal(rp['counts'], plain['counts'])
    assert np.array_equal(rp['turbo_iters_hist'], plain['turbo_iters_hist'])
    hist = plain['turbo_iters_hist']
    assert hist[:, 2:].sum() > 0 and hist[:, 1].sum() > 0            # blocks on both sides of the boundary
    parts = [call(repack=True, rank=k, world_size=2) for k in range(2)]       # True: the default boundary, 1
    assert parts[0]['plan'] is rp['plan']
    assert np.array_equal(parts[0]['counts'] + parts[1]['counts'], rp['counts'])
    assert np.array_equal(parts[0]['turbo_iters_hist'] + parts[1]['turbo_iters_hist'], rp['turbo_iters_hist'])


# ---------------------------------------------------------------------------
# (6) switching and refusals
def own_plan(C, **kw):
    """A plan of this test's own (not get_plan's cache): K = 40, QPSK on AWGN."""
    from lte_phy import engine
    base = dict(N=128, Nc=72, cp_len=9, bps=2, n_sym=0, chain=C.CHAIN_CODED, channel=C.CH_AWGN, fs=1.92e6, n_bits=16,
                max_frames=FRAMES, turbo_iters=ITERS)
    return engine.Plan(**dict(base, **kw))


def test_switching(C):
    lib = C.load()
    snrs = np.where(np.arange(FRAMES) % 4 == 1, np.linspace(-5.0, 3.0, FRAMES), 9.0)
    kw = dict(seed=5, frame_ids=np.arange(FRAMES, dtype=np.uint64), capture=('bits_rx',))
    plain, p = own_plan(C, early_stop=True), own_plan(C, early_stop=True, repack=2)
    a = plain.run(snrs, **kw)
    b = p.run(snrs, **kw)
    assert b.path['repack'] == '2' and b['repack_info'] == expected_info(a['turbo_iters_used'], 2, CAP)
    assert 'packed' in b['repack_info']['state']
    p.set_repack(0)                                                 # off again: the plain path and results
    assert lib.lte_plan_early_stop_repack(p.h) == 0 and lib.lte_plan_early_stop(p.h) == 1
    info = np.zeros(5, dtype=np.int64)
    assert lib.lte_plan_repack_info(p.h, C.ptr(info, C.c_i64), 5) == C.LTE_EINVAL
    c = p.run(snrs, **kw)
    assert c.path == a.path and 'repack_info' not in c
    p.set_repack(True)
    assert lib.lte_plan_early_stop_repack(p.h) == 1
    d = p.run(snrs, **kw)
    assert d['repack_info'] == expected_info(a['turbo_iters_used'], 1, CAP)
    for k in SAME:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) and np.array_equal(a[k], d[k]), k
    # lte_plan_repack_info: the full length, cut to n
    assert lib.lte_plan_repack_info(p.h, C.ptr(info, C.c_i64), 3) == 5
    assert info.tolist() == [1, 1, d['repack_info']['undecided'][0], 0, 0]
    for bad in (-1, ITERS, ITERS + 1):
        assert lib.lte_plan_set_early_stop_repack(p.h, bad) == C.LTE_EINVAL
    assert lib.lte_plan_early_stop_repack(p.h) == 1
    assert lib.lte_plan_set_early_stop(p.h, 0) == C.LTE_OK          # clears re-packing too
    assert lib.lte_plan_early_stop_repack(p.h) == 0
    assert lib.lte_plan_set_early_stop_repack(p.h, 1) == C.LTE_EINVAL
    assert lib.lte_plan_set_early_stop(p.h, 1) == C.LTE_OK and lib.lte_plan_early_stop_repack(p.h) == 0


def test_fixed_and_harq_plans_refuse_the_setter(C):
    lib = C.load()
    for plan in (own_plan(C), own_plan(C, harq=dict(max_tx=2, rv_seq=(0, 2)))):
        assert lib.lte_plan_set_early_stop_repack(plan.h, 1) == C.LTE_EINVAL
        assert lib.lte_plan_set_early_stop_repack(plan.h, 0) == C.LTE_EINVAL
        assert lib.lte_plan_early_stop_repack(plan.h) == 0


def test_exact_logmap_is_refused(C, cc, oracle):
    p = own_plan(C, early_stop=True, repack=1)
    llr = stage_pool(oracle, 40, '24B', False)[0]
    try:
        cc.set_decoder_mode(False)
        with pytest.raises(NotImplementedError, match='max-log'):       # LTE_EUNSUP (_capi.check)
            p.run(np.full(4, 9.0), seed=1)
        with pytest.raises(NotImplementedError, match='max-log'):
            cc.turbo_decode_early_stop(llr, 40, ITERS, '24B', repack=1)
    finally:
        cc.set_decoder_mode(True)
    assert 'repack_info' in p.run(np.full(4, 9.0), seed=1)


# ---------------------------------------------------------------------------
# (7) device memory
def test_packed_arrays_are_counted(C):
    lib = C.load()
    start = int(lib.lte_device_bytes_held())
    p = own_plan(C, early_stop=True)
    before = int(lib.lte_device_bytes_held())
    p.set_repack(1)
    K, cap = 40, CAP
    # per slot: rows, checkpoints (K / 8 + 1 windows of 8 states), decision words, counts, indices; the slot counts
    want = cap * 64 * ((4 * K + 12) * 8 + (K // 8 + 1) * 8 * 8 + 2 * 4 + 4 + 4) + 4
    assert int(lib.lte_device_bytes_held()) - before == want
    p.set_repack(0)
    p.set_repack(2)                                                  # off and on again: nothing freed, nothing more
    assert int(lib.lte_device_bytes_held()) - before == want
    assert lib.lte_plan_destroy(p.h) == C.LTE_OK
    p.h = None
    assert int(lib.lte_device_bytes_held()) == start
