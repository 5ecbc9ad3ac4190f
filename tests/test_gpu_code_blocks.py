"""GPU: the channel-coding kernels over all 188 code-block sizes and the coded
chain over a ladder of transport-block sizes, against the float64 oracle
(oracle/lte_oracle.py, itself pinned to the reference's goldens and, for the
tables of every size, to tests/golden/golden_cb_tables.json by
tests/test_code_block_tables.py).

  (a) k_encode through lte_turbo_encode_host, every K, exact
  (b) k_turbo64 / k_turbo through turbo_decode_batch, every K, 2 iterations,
      bit-exact vs the float64 decoder / the float32 model, on blocks the
      oracle itself fails to decode (2 dB) and decodes (4 dB)
  (c) k_turbo64_logmap, one K per (K % 32, K % 24) class of each table
      granularity, decisions vs a NumPy log-MAP restatement
  (d) the rate-dematch kernel through rate_dematching_turbo, one K per K % 32
      class of each granularity, puncturing and repetition, exact
  (e) the whole coded chain at TB sizes chosen for their K / filler / word
      count (EXPECT below, asserted per case), 67 frames, f64 and f32, on the
      LLR path (k_dematch) and the symbol hand-off (k_dematch_zn)
  (f) two of those cases under each transmitter / receiver switch
  (g) the library's own segmentation (lte_plan_create) at the reference's
      boundary sizes

The 188 sizes are split into 8 chunks, each a stride of the sorted list, so
every chunk spans small and large K (below 528, where the sizes step by 8, a
chunk steps by 64 and so stays in one K % 32 class; the 8 chunks together hold
every size).  Everything is exact except tx_syms in float32 (1e-6, the suite's
tolerance for it)."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TAB = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'golden_cb_tables.json')))
SIZES = TAB['sizes']
N_CHUNKS = 8
FRAMES = 64 + 3          # one full 64-frame decoder group and a partial one
ITERS = 2                # DEC1 -> DEC2 -> DEC1 -> DEC2 -> FINAL: every half-pass mode and the first-pass flag
SWITCHES = ('LTE_TXCH_FUSE', 'LTE_RX_FUSE', 'LTE_TX_FRAME', 'LTE_RX_WAVE', 'LTE_TX_WAVE', 'LTE_DEMAP_IN_DEMATCH',
            'LTE_TXW_STAGE', 'LTE_TX_STAGE')


def chunk(c):
    return SIZES[c::N_CHUNKS]


assert sorted(K for c in range(N_CHUNKS) for K in chunk(c)) == SIZES and len(SIZES) == 188


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
# (a) encoder
def _encode(C, bits):
    n, K = bits.shape
    out = np.zeros((n, 3 * K + 12), dtype=np.uint8)
    C.check(C.load().lte_turbo_encode_host(K, n, C.ptr(bits, C.U8), C.ptr(out, C.U8)))
    return out


@pytest.mark.parametrize('c', range(N_CHUNKS))
def test_encoder_every_size(C, oracle, c):
    """k_encode, 3 random blocks per K: the partial last word (K % 32 = 8, 16,
    24), blocks of fewer than 4 words (empty encoder waves) and the QPP walk of
    every row of QPP_TAB."""
    for K in chunk(c):
        bits = np.random.RandomState(K).randint(0, 2, (3, K)).astype(np.uint8)
        out = _encode(C, bits)
        for i in range(3):
            assert np.array_equal(out[i], oracle.turbo_encode(bits[i])), (K, i)


@pytest.mark.parametrize('K', [56, 88, 120, 6144])
def test_encoder_partial_lane_group(C, oracle, K):
    """64 + 3 blocks of one K: the second 64-lane group is partial.  56, 88 and
    120 are the sizes with K % 32 = 24 and fewer than 4 words."""
    n = 64 + 3
    bits = np.random.RandomState(1000 + K).randint(0, 2, (n, K)).astype(np.uint8)
    out = _encode(C, bits)
    for i in range(n):
        assert np.array_equal(out[i], oracle.turbo_encode(bits[i])), (K, i)


# ---------------------------------------------------------------------------
# (b) decoders
DEC_SNR = (2.0, 4.0, 4.0)    # block 0 below the cliff at 2 iterations, blocks 1 and 2 above it
DEC_SEED = 0                 # added to K: move it, never the condition, if a chunk misses the condition
_DEC = {}


def decoder_inputs(O, K):
    """(code blocks [3][K], LLRs [3][3K + 12]) as test_turbo_decode_batch_vs_oracle
    builds them, from RandomState(K)."""
    if K not in _DEC:
        rs = np.random.RandomState(K + DEC_SEED)
        cbs = rs.randint(0, 2, (len(DEC_SNR), K)).astype(np.uint8)
        llr = np.zeros((len(DEC_SNR), 3 * K + 12))
        for i, snr in enumerate(DEC_SNR):
            s2 = 10 ** (-snr / 10)
            s = 1 - 2.0 * O.turbo_encode(cbs[i])
            llr[i] = 2 * (s + np.sqrt(s2) * rs.randn(len(s))) / s2
        _DEC[K] = (cbs, llr)
    return _DEC[K]


def check_sensitivity(fails):
    """fails [n_K][3] (oracle decision != sent block): over a chunk the oracle
    fails at least 25 % of the 2 dB blocks -- the ones whose decisions react to
    any wrong extrinsic -- and decodes at least 75 % of the 4 dB blocks."""
    fails = np.asarray(fails)
    lo, hi = fails[:, 0], fails[:, 1:]
    assert lo.mean() >= 0.25, ('2 dB blocks the oracle fails', int(lo.sum()), lo.size)
    assert 1 - hi.mean() >= 0.75, ('4 dB blocks the oracle decodes', int(hi.size - hi.sum()), hi.size)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('c', range(N_CHUNKS))
def test_decoder_every_size(cc, oracle, c, prec):
    """k_turbo64 (f64) == the reference's float64 decoder and k_turbo (f32) ==
    its float32 model, bit for bit on every block of every K: 8-step windows in
    16-step (f32) / 24-step (f64) super-windows with every remainder, hard
    decisions packed across 32-bit boundaries, the modular QPP walk forwards
    and backwards for every (f1, f2) row."""
    fails = []
    for K in chunk(c):
        cbs, llr = decoder_inputs(oracle, K)
        if prec == 'f64':
            dec = cc.turbo_decode_batch(llr, K, ITERS)
            ref = [oracle.turbo_decode(llr[i], K, ITERS) for i in range(len(llr))]
        else:
            l32 = llr.astype(np.float32)
            dec = cc.turbo_decode_batch(l32, K, ITERS, precision='f32')
            ref = [oracle.turbo_decode_f32_model(l32[i], K, ITERS) for i in range(len(llr))]
        for i in range(len(llr)):
            assert np.array_equal(dec[i], ref[i]), (K, i, int(np.sum(dec[i] != ref[i])))
        fails.append([bool(np.any(ref[i] != cbs[i])) for i in range(len(llr))])
    check_sensitivity(fails)


# ---------------------------------------------------------------------------
# (c) exact log-MAP
# the largest K of every (K % 32, K % 24) class within each granularity of the
# size table (8 up to 512: 12 classes, 16 up to 1024: 6, 32 up to 2048: 3, 64
# up to 6144: 3), and the four smallest sizes (less than one super-window)
LOGMAP_K = [40, 48, 56, 64,
            424, 432, 440, 448, 456, 464, 472, 480, 488, 496, 504, 512,
            944, 960, 976, 992, 1008, 1024,
            1984, 2016, 2048,
            6016, 6080, 6144]


def test_logmap_sizes_cover_every_class():
    for lo, hi, n in [(40, 512, 12), (528, 1024, 6), (1056, 2048, 3), (2112, 6144, 3)]:
        every = {(K % 32, K % 24) for K in SIZES if lo <= K <= hi}
        assert len(every) == n and {(K % 32, K % 24) for K in LOGMAP_K if lo <= K <= hi} == every


def lse(a, b):
    """channel_coding.log_sum_exp (turbo_decoder.py:64-88) on arrays."""
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid='ignore'):
        out = hi + np.log1p(np.exp(lo - hi))
    return np.where(np.isneginf(lo), hi, out)


def _trellis():
    ns, sy, pa = np.zeros((8, 2), dtype=int), np.zeros((8, 2)), np.zeros((8, 2))
    for s in range(8):
        s0, s1, s2 = (s >> 2) & 1, (s >> 1) & 1, s & 1
        for u in range(2):
            fb = (u + s1 + s2) % 2
            ns[s, u], sy[s, u], pa[s, u] = (fb << 2) | (s0 << 1) | s1, fb, (fb + s0 + s2) % 2
    return ns, 1 - 2 * sy, 1 - 2 * pa


def bcjr_logmap(ls, lp, la):
    """LogMAPDecoder.decode (turbo_decoder.py:181-278) with max* = log_sum_exp,
    a-posteriori LLRs; [n][steps] arrays, the recursions vectorised over blocks
    and states, accumulated in the reference's order."""
    ns, sgn_s, sgn_p = _trellis()
    n, T = ls.shape
    sgn_u = np.array([1.0, -1.0])
    gamma = (ls[:, :, None, None] / 2.0 * sgn_s + lp[:, :, None, None] / 2.0 * sgn_p) + \
        la[:, :, None, None] / 2.0 * sgn_u                                             # [n][T][8][2]
    inc = [[(s, u) for s in range(8) for u in range(2) if ns[s, u] == t] for t in range(8)]
    in0 = np.array([2 * i[0][0] + i[0][1] for i in inc])
    in1 = np.array([2 * i[1][0] + i[1][1] for i in inc])
    alpha = np.full((n, T + 1, 8), -np.inf)
    beta = np.full((n, T + 1, 8), -np.inf)
    alpha[:, 0, 0] = 0.0
    beta[:, T, 0] = 0.0
    for k in range(T):
        v = (alpha[:, k, :, None] + gamma[:, k]).reshape(n, 16)
        alpha[:, k + 1] = lse(v[:, in0], v[:, in1])
    for k in range(T - 1, -1, -1):
        v = beta[:, k + 1][:, ns] + gamma[:, k]
        beta[:, k] = lse(v[:, :, 0], v[:, :, 1])
    val = alpha[:, :T, :, None] + gamma + beta[:, 1:][:, :, ns]                        # [n][T][8][2]
    l0 = l1 = np.full((n, T), -np.inf)
    for s in range(8):
        l0, l1 = lse(l0, val[:, :, s, 0]), lse(l1, val[:, :, s, 1])
    return l0 - l1


def turbo_decode_logmap(O, llr, K, iters):
    """turbo_decode (turbo_decoder.py:338-450) on [n][3K + 12] LLRs."""
    perm = O.qpp_perm(K)
    inv = np.argsort(perm)
    n = llr.shape[0]
    z3 = np.zeros((n, 3))
    sy, p1, p2 = llr[:, 0:3 * K:3], llr[:, 1:3 * K:3], llr[:, 2:3 * K:3]
    ls1 = np.concatenate([sy, llr[:, 3 * K:3 * K + 3]], axis=1)
    lp1 = np.concatenate([p1, llr[:, 3 * K + 3:3 * K + 6]], axis=1)
    ls2 = np.concatenate([sy[:, perm], llr[:, 3 * K + 6:3 * K + 9]], axis=1)
    lp2 = np.concatenate([p2, llr[:, 3 * K + 9:3 * K + 12]], axis=1)
    e21 = np.zeros((n, K))
    for _ in range(iters):
        la = np.concatenate([e21, z3], axis=1)
        e12 = (bcjr_logmap(ls1, lp1, la) - la - ls1)[:, :K]
        la = np.concatenate([e12[:, perm], z3], axis=1)
        e21 = (bcjr_logmap(ls2, lp2, la) - la - ls2)[:, :K][:, inv]
    app = bcjr_logmap(ls1, lp1, np.concatenate([e21, z3], axis=1))
    return (app[:, :K] < 0).astype(np.uint8), app[:, :K]


def test_lse_is_log_sum_exp(cc):
    a = np.array([-np.inf, 0.5, -np.inf, 3.0, -2.0, 1e3, 0.0])
    b = np.array([1.5, -np.inf, -np.inf, 3.0, 7.25, -1e3, 1e-9])
    assert np.array_equal(lse(a, b), np.array([cc.log_sum_exp(x, y) for x, y in zip(a, b)]))


@pytest.mark.parametrize('K', LOGMAP_K)
def test_logmap_decoder(cc, oracle, K):
    """set_decoder_mode(False), float64, 1 iteration, a 2 dB and a 4 dB block:
    k_turbo64_logmap's decisions == the NumPy restatement's.  The two evaluate
    exp / log1p with different libm, so a-posteriori LLRs agree to round-off
    only: a decision may legitimately differ only where the restatement's LLR
    is within that round-off of zero, which the test rules out first."""
    cbs, llr = decoder_inputs(oracle, K)
    llr = llr[:2]
    ref, app = turbo_decode_logmap(oracle, llr, K, 1)
    assert np.min(np.abs(app)) > 1e-9 * np.max(np.abs(app))
    try:
        cc.set_decoder_mode(False)
        dec = cc.turbo_decode_batch(llr, K, 1)
    finally:
        cc.set_decoder_mode(True)
    assert np.array_equal(dec, ref), (K, int(np.sum(dec != ref)))
    maxlog = np.stack([oracle.turbo_decode(llr[i], K, 1) for i in range(2)])
    assert np.array_equal(cc.turbo_decode_batch(llr, K, 1), maxlog)      # the mode was restored


# ---------------------------------------------------------------------------
# (d) rate dematch kernel
# one K per K % 32 class at the ends of each granularity of the size table
DEMATCH_K = [40, 48, 56, 64, 504, 512, 528, 1008, 1024, 1056, 2016, 2112, 6080, 6144]
RM_SHAPES = [(lambda K: 3 * K + 12, 0), (lambda K: K + 17, 2), (lambda K: 2 * K + 5, 1), (lambda K: 4 * K, 3)]


@pytest.mark.parametrize('K', DEMATCH_K)
def test_rate_dematch_kernel(cc, oracle, K):
    """rate_dematching_turbo on the GPU: full buffer (rv 0), puncturing (rv 2,
    rv 1) and repetition E = 4K > N_cb (rv 3: repeats summed in order)."""
    rs = np.random.RandomState(K)
    for fE, rv in RM_SHAPES:
        x = rs.randn(fE(K))
        assert np.array_equal(cc.rate_dematching_turbo(x, K, rv), oracle.rate_dematch(x, K, rv)), (K, fE(K), rv)


# ---------------------------------------------------------------------------
# (e) TB-size ladder through the coded chain
# n_bits -> (words of the TB with CRC-24A, [(K, F) per code block]): what each
# size is in the ladder for.  Asserted against the oracle's plan in every case.
EXPECT = {
    1: (1, [(40, 15)]),              # less than one word, 2-word block, two empty encoder waves, filler
    16: (2, [(40, 0)]),
    17: (2, [(48, 7)]),              # K % 32 = 16 below 4 words
    25: (2, [(56, 7)]),              # K % 32 = 24
    39: (2, [(64, 1)]),
    73: (4, [(104, 7)]),             # K % 32 = 8
    435: (15, [(464, 5)]),           # K % 32 = 16
    500: (17, [(528, 4)]),           # K % 32 = 16, first size of the 16 granularity
    1001: (33, [(1056, 31)]),
    2041: (65, [(2112, 47)]),
    6057: (191, [(6144, 63)]),       # the largest block with the most filler
    6120: (192, [(6144, 0)]),
    6121: (193, [(3072, 0), (3136, 15)]),                 # the first two-block TB, filler in block 1
    12217: (383, [(4096, 0), (4096, 0), (4160, 39)]),
}
# snr: the frames' SNRs are linspace(lo, hi, 67), chosen on the CPU (oracle.simulate_siso_coded at 2
# iterations) so that the oracle passes and fails at least MIN_PASS / MIN_FAIL frames with room to
# spare.  Blocks of 40..64 bits with filler are much stronger codes than their nominal rate (a 1-bit
# TB never fails at -2 dB), so the AWGN ladder starts lower for them: -8..8 dB gives 22..37 failing
# and 30..45 passing frames, -2..10 dB at the larger sizes 23..37 and 30..44, 0..30 dB on the
# Rayleigh ladder 16..27 and 40..51.
LADDER_A = dict(bw=1.25, mod='QPSK', chan='awgn', snr=(-2.0, 10.0), snr_small=(-8.0, 8.0),
                sizes=[1, 16, 17, 25, 39, 73, 435, 500, 1001, 2041, 6057, 6120, 6121])
LADDER_B = dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', snr=(0.0, 30.0), sizes=[17, 73, 435, 2041, 6121, 12217])
LADDERS = {'A': LADDER_A, 'B': LADDER_B}
MIN_PASS = MIN_FAIL = 4


def ladder_inputs(n_bits, lad):
    bits = np.random.RandomState(n_bits).randint(0, 2, (FRAMES, n_bits)).astype(np.uint8)
    lo, hi = lad.get('snr_small', lad['snr']) if n_bits < 64 else lad['snr']
    return bits, np.linspace(lo, hi, FRAMES)


def coded_qam(O, num, bits):
    """The QAM symbols oracle.coded_tx maps and where the T/F interleaver puts
    them in the grid (core/ofdm_core.py:1003-1060), without its OFDM modulation."""
    cbs, plan = O.segment(O.attach_crc24a(bits))
    coded = np.concatenate([O.rate_match(O.turbo_encode(cb), 3 * len(cb) + 12, len(cb), 0) for cb in cbs])
    qam = O.bits_to_symbols(coded, num.modulation)
    q = np.arange(len(qam))
    rows = -(-len(qam) // num.Nd)
    return qam, (q % num.Nd) * rows + q // num.Nd, plan


def ladder_plan(C, O, lad, prec, n_bits):
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=lad['bw'], modulation=lad['mod']),
                                channel_type=lad['chan'], precision=prec)
    plan = sim._plan(C.CHAIN_CODED, 0, n_bits, max_frames=FRAMES, iters=ITERS)
    num = O.Numerology(bandwidth=lad['bw'], modulation=lad['mod'])
    seg = O.segmentation_plan(n_bits + 24)
    words, kf = EXPECT[n_bits]
    assert [(p[0], p[1]) for p in seg] == kf and -(-(n_bits + 24) // 32) == words
    assert plan.n_cb == len(kf) and plan.coded_bits == sum(3 * K + 12 for K, _ in kf)
    assert plan.Nd == num.Nd
    return plan, num, seg


def check_run1(O, plan, num, seg, r, bits, prec, tag):
    """Run 1's assertions: transmitted symbols, the oracle's RX decode of the
    run's own LLRs, per-frame error counts; returns the oracle's CRC verdicts."""
    bps, Nd, coded = num.bps, num.Nd, plan.coded_bits
    ncs = coded // bps
    rows = -(-ncs // Nd)
    q = np.arange(ncs)
    src_re = (q % Nd) * rows + q // Nd
    rm = [3 * p[0] + 12 for p in seg]
    oks = []
    for b in range(FRAMES):
        qam, pos, _ = coded_qam(O, num, bits[b])
        ts = r['tx_syms'][b].astype(np.complex128)[pos]
        if prec == 'f64':
            assert np.array_equal(ts, qam), (tag, b)
        else:
            assert np.max(np.abs(ts - qam)) < 1e-6, (tag, b)
        L = r['llr'][b].astype(np.float64).reshape(-1, bps)[src_re].reshape(-1)[:coded]
        dec, ok = O.coded_rx_decode(L, seg, rm, ITERS, f32_model=(prec == 'f32'))
        assert np.array_equal(dec, r['bits_rx'][b]), (tag, b, int(np.sum(dec != r['bits_rx'][b])))
        assert bool(ok) == bool(r['crc_ok'][b]), (tag, b)
        assert int(r['frame_errors'][b]) == int(np.sum(bits[b] != r['bits_rx'][b])), (tag, b)
        oks.append(bool(ok))
    n_ok = sum(oks)
    assert n_ok >= MIN_PASS and FRAMES - n_ok >= MIN_FAIL, (tag, n_ok)
    return oks


def clear_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


CAP1 = ('tx_syms', 'llr', 'bits_rx')
LADDER_CASES = [(name, n) for name in ('A', 'B') for n in LADDERS[name]['sizes']]


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('ladder,n_bits', LADDER_CASES)
def test_chain_tb_ladder(C, oracle, monkeypatch, ladder, n_bits, prec):
    """One TB size through k_payload / k_encode / TX / channel / RX / k_dematch
    (or k_dematch_zn) / k_turbo* / k_crc_count, 67 frames spread over the turbo
    cliff.  Run 1 (injected bits, LLRs captured): see check_run1.  Run 2 (no
    LLR capture: 16-QAM demaps inside the dematch): identical decisions.  Run 3
    (AWGN ladder: the kernel's own Philox payload at 30 dB): every frame passes
    its CRC with no bit error, which ties k_payload's CRC tree to k_crc_count's
    re-draw of the payload."""
    clear_switches(monkeypatch)
    lad = LADDERS[ladder]
    plan, num, seg = ladder_plan(C, oracle, lad, prec, n_bits)
    bits, snrs = ladder_inputs(n_bits, lad)
    tag = f'{ladder}/{n_bits}/{prec}'
    r1 = plan.run(snrs, seed=n_bits, bits=bits, capture=CAP1)
    assert r1.path['dematch'] == 'llr'
    assert np.array_equal(coded_qam(oracle, num, bits[0])[0], oracle.coded_tx(num, bits[0])['qam'])
    check_run1(oracle, plan, num, seg, r1, bits, prec, tag)
    r2 = plan.run(snrs, seed=n_bits, bits=bits, capture=('bits_rx',))
    assert r2.path['dematch'] == ('zn' if num.bps > 2 else 'llr')
    assert path_diff(r1.path, r2.path) <= {'dematch', 'rx'}, (r1.path, r2.path)
    for k in ('bits_rx', 'crc_ok', 'frame_errors'):
        assert np.array_equal(r1[k], r2[k]), (tag, k, np.flatnonzero(np.any(np.atleast_2d(r1[k].T != r2[k].T), axis=0)))
    if lad['chan'] == 'awgn':
        r3 = plan.run(np.full(FRAMES, 30.0), seed=1 + n_bits)
        assert np.array_equal(r3['crc_ok'], np.ones(FRAMES, dtype=np.uint8)), (tag, np.flatnonzero(r3['crc_ok'] == 0))
        assert not r3['frame_errors'].any(), (tag, r3['frame_errors'])
        assert int(r3['counts'][0, 0]) == 0 and int(r3['counts'][0, 2]) == 0     # bit errors, block errors


def path_diff(a, b):
    from lte_phy.engine import path_diff as diff
    return diff(a, b)


# ---------------------------------------------------------------------------
# (f) path switches
# label -> (environment, the run it is compared with, the path fields that move
# and their new values).  5 MHz is N = 512: the per-frame transmitter
# k_ofdm_txf is the default, LTE_TX_STAGE only reaches the per-symbol
# transmitters (so it is flipped on top of LTE_TX_FRAME=0), and the wave
# transmitter needs N = 2048 (txf_w_supported), so LTE_TX_WAVE=1 must leave the
# path alone here.
VARIANTS = {
    'tx_frame0': ({'LTE_TX_FRAME': '0'}, {}, {'tx': 'k_ofdm_tx_ch'}),
    'tx_stage0': ({'LTE_TX_FRAME': '0', 'LTE_TX_STAGE': '0'}, {'LTE_TX_FRAME': '0'}, {'tx_stage': '0'}),
    'tx_wave1': ({'LTE_TX_WAVE': '1'}, {}, {}),
    'txch_fuse0': ({'LTE_TXCH_FUSE': '0'}, {}, {'tx': 'k_ofdm_tx', 'ch_fix': '0'}),
    'rx_fuse0': ({'LTE_RX_FUSE': '0'}, {}, {'rx': 'k_rx_chest+k_rx_data'}),
}


@pytest.mark.parametrize('label', list(VARIANTS))
@pytest.mark.parametrize('n_bits', [73, 6121])
def test_chain_tb_ladder_path_switches(C, oracle, monkeypatch, n_bits, label):
    """Run 1 of two ladder-B cases (f64) on the other transmitters and the
    separate receiver kernels: the same assertions hold on each path."""
    clear_switches(monkeypatch)
    lad, prec = LADDER_B, 'f64'
    plan, num, seg = ladder_plan(C, oracle, lad, prec, n_bits)
    bits, snrs = ladder_inputs(n_bits, lad)
    env, base_env, moved = VARIANTS[label]
    kw = dict(seed=n_bits, bits=bits, capture=CAP1)
    for k, v in base_env.items():
        monkeypatch.setenv(k, v)
    base = plan.path(snrs, **kw)
    assert (base['rx'], base['ch_fix'], base['dematch']) == ('k_rx_frame', '1', 'llr'), base
    assert base['tx'] == ('k_ofdm_tx_ch' if base_env else 'k_ofdm_txf'), base
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = plan.run(snrs, **kw)
    diff = path_diff(base, r.path)
    # tx_stage describes the transmitter in use: it may move with 'tx'
    assert set(moved) <= diff <= set(moved) | ({'tx_stage'} if 'tx' in moved else set()), (label, base, r.path)
    assert all(r.path[k] == v for k, v in moved.items()), (label, r.path)
    check_run1(oracle, plan, num, seg, r, bits, prec, f'B/{n_bits}/{label}')


# ---------------------------------------------------------------------------
# (g) the library's segmentation
def test_plan_segmentation_boundaries(C):
    """lte_plan_create's segmentation_plan (lte_capi.hip) at the reference's
    boundary sizes of C = 1..13 blocks and the ends of the size table: block
    count and total coded bits equal get_segmentation_info of the reference."""
    import lte_phy
    from lte_phy import engine
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=20.0, modulation='64-QAM'), channel_type='awgn')
    rows = [r for r in TAB['seg_info'] if r[0] > 6144 or r[0] in (25, 39, 40, 41, 6143, 6144)]
    assert {r[1] for r in rows} == set(range(1, 14)) and len(rows) <= 48
    for B, n, sizes, total in rows:
        plan = sim._plan(C.CHAIN_CODED, 0, B - 24, max_frames=1)
        assert (plan.n_cb, plan.coded_bits) == (n, total), (B, sizes)
        del plan
    engine.clear_cache()
