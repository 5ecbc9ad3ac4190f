"""Exact-input LLR pools for the turbo decoders (a helper, not a conftest).

On LLRs that are small multiples of a power of two, every gamma, alpha, beta,
extrinsic and a-posteriori L of max-log-MAP is a small multiple of one quantum
q, so it is exactly representable in float32 as well as in float64: the
float32 decoders' normalisation (a subtraction of such values) is exact, and so
is a multiplication by the scale 0.5.  Any correct evaluation order then gives
the float64 reference's result bit for bit, so on these pools the float32
kernels -- and their C models -- must equal oracle.turbo_decode itself, below
the cliff as well as above it.  Quantised LLRs also tie (L == 0 exactly) and
hold exact zeros by the thousand, which continuous Gaussian LLRs never do.

  pool(O, K, step, clip, erase)   the blocks of one size and quantisation
  exactness_audit(O, llr, K, iters, scale)
                                  a plain float64 NumPy max-log evaluation that
                                  checks the premise (every value a multiple of
                                  q, far below 2^24 q) instead of assuming it
  reference(O, K, quant)          the reference's D(0) .. D(8) of every block
  lanes / pool_conditions / assert_pool_conditions
                                  the 131-lane layout and the conditions under
                                  which a wrong kernel could not pass

tests/test_exact_llr_host.py checks the models and the conditions on the CPU,
tests/test_gpu_exact_llr.py the kernels.
"""
import collections

import numpy as np

import turbo_scaled_model as M

POLYS = M.POLYS
ITERS = 8                      # unscaled decodes
SC_SCALE, SC_ITERS = 0.5, 4    # scaled decodes: 8 halvings of the quantum; 0.75 is not exact (x 3 per half-iteration)
NCB = 2 * 64 + 3
RATIO_BOUND = 2.0 ** 22        # a factor 4 under float32's 2^24: the kernel forms three-term sums before it normalises
KS = (40, 56, 64, 1056, 6144)  # the geometry set of turbo_scaled_model.STAGE (48 adds no window case to 40 / 56)
# name -> (step, clip, erased fraction)
QUANT = {'s1': (1.0, 7.0, 0.0), 's025': (0.25, 31.75, 0.0), 's2e': (2.0, 6.0, 0.25)}
# K -> (lo, hi, blocks) of the ladder of per-block SNRs in dB, spanning the
# cliff of that K for the quantised BPSK LLRs (at 8 iterations the reference's
# cliff is near 3 dB for 1056 and 6144, and between 0 and 4 dB for the short
# blocks).  Step 2.0 with clip 6 and 25 % erasures moves it up by ERASED_SHIFT.
LADDER = {40: (-1.0, 5.0, 44), 56: (-1.0, 5.0, 44), 64: (-1.0, 5.0, 44), 1056: (2.0, 4.25, 26), 6144: (2.0, 4.5, 18)}
ERASED_SHIFT = 3.0


def ladder(K, erase=0.0):
    lo, hi, n = LADDER[K]
    return np.linspace(lo, hi, n) + (ERASED_SHIFT if erase else 0.0)


# (K, quantisation) -> seed: moved (never a condition) until assert_pool_conditions holds
SEED = {(40, 's1'): 3, (40, 's025'): 3, (40, 's2e'): 1, (56, 's1'): 11, (56, 's025'): 6, (56, 's2e'): 4,
        (64, 's1'): 3, (64, 's025'): 1, (64, 's2e'): 1, (1056, 's1'): 0, (1056, 's025'): 0, (1056, 's2e'): 0,
        (6144, 's1'): 0, (6144, 's025'): 0, (6144, 's2e'): 0}

ZERO, NOPAR, CLIP_A, CLIP_A_NOSYS, CLIP_B, CLIP_B_NOSYS = 1, 2, 3, 4, 5, 6   # Pool.kind of the known-answer blocks
Pool = collections.namedtuple('Pool', 'llr sent crc kind')
_POOL, _REF, _SC, _TIES = {}, {}, {}, {}


def quantise(llr, step, clip):
    return np.clip(np.rint(np.asarray(llr, dtype=np.float64) / step) * step, -clip, clip)


def pool(O, K, step, clip, erase, seed=0):
    """Distinct blocks of one K: a random payload with its CRC-24 (24B for even
    blocks, 24A for odd ones), turbo-encoded, BPSK LLRs 2y / s2 at the block's
    own SNR, rounded to `step`, clipped to +-clip, a fraction `erase` set to
    exactly 0.0.  Then the known-answer blocks, whose outputs follow without a
    decoder:
      ZERO          every LLR 0.0: every L is exactly 0, D(n) is all zeros, n* = 1
      NOPAR         parity and tail LLRs 0.0, the systematic ones quantised
      CLIP_A / _B   every |LLR| = clip with the sent signs (CRC-24A / -24B word)
      *_NOSYS       the same with the K systematic LLRs erased
    Pool(llr [n][3K + 12] float64, sent [n][K], crc [n] '24A' / '24B' / '', kind [n])."""
    key = (K, step, clip, erase, seed)
    if key not in _POOL:
        rs = np.random.RandomState(100003 * seed + K)
        llr, sent, crc, kind = [], [], [], []

        def word(gen):
            p = rs.randint(0, 2, K - 24).astype(np.uint8)
            return np.concatenate([p, O.crc_bits(p, POLYS[gen], 24)])

        for i, snr in enumerate(ladder(K, erase)):
            gen = '24B' if i % 2 == 0 else '24A'
            cb = word(gen)
            s2 = 10 ** (-snr / 10)
            y = 1 - 2.0 * O.turbo_encode(cb) + np.sqrt(s2) * rs.randn(3 * K + 12)
            q = quantise(2 * y / s2, step, clip)
            q[rs.rand(3 * K + 12) < erase] = 0.0
            llr.append(q), sent.append(cb), crc.append(gen), kind.append(0)
        sys_pos = np.arange(0, 3 * K, 3)
        llr.append(np.zeros(3 * K + 12)), sent.append(np.zeros(K, dtype=np.uint8)), crc.append(''), kind.append(ZERO)
        cb = word('24B')
        q = np.zeros(3 * K + 12)
        q[sys_pos] = quantise(2 * (1 - 2.0 * cb + rs.randn(K)), step, clip)
        llr.append(q), sent.append(cb), crc.append(''), kind.append(NOPAR)
        for gen, k_full, k_nosys in (('24A', CLIP_A, CLIP_A_NOSYS), ('24B', CLIP_B, CLIP_B_NOSYS)):
            cb = word(gen)
            q = clip * (1 - 2.0 * O.turbo_encode(cb))
            llr.append(q), sent.append(cb), crc.append(gen), kind.append(k_full)
            q = q.copy()
            q[sys_pos] = 0.0
            llr.append(q), sent.append(cb), crc.append(gen), kind.append(k_nosys)
        _POOL[key] = Pool(np.array(llr) + 0.0, np.array(sent), np.array(crc), np.array(kind))   # + 0.0: no -0.0
    return _POOL[key]


def quant_pool(O, K, quant):
    return pool(O, K, *QUANT[quant], seed=SEED[(K, quant)])


# ---------------------------------------------------------------------------
# The audit: max-log-MAP in float64 NumPy, vectorised over blocks and states,
# with the reference's unnormalised recursions (alpha / beta start at delta_0 /
# -inf) so that every intermediate value can be inspected.
def _trellis():
    NS, FB, PAR = np.zeros((8, 2), int), np.zeros((8, 2), int), np.zeros((8, 2), int)
    for s in range(8):
        s0, s1, s2 = s >> 2, (s >> 1) & 1, s & 1
        for u in range(2):
            fb = u ^ s1 ^ s2
            NS[s, u], FB[s, u], PAR[s, u] = 4 * fb + 2 * s0 + s1, fb, fb ^ s0 ^ s2
    pre = [[(s, u) for s in range(8) for u in range(2) if NS[s, u] == ns] for ns in range(8)]
    PRE = np.array([[2 * s + u for s, u in p] for p in pre])           # flat (s, u) of the two branches into ns
    return NS, 1 - 2.0 * FB, 1 - 2.0 * PAR, PRE


_NS, _SFB, _SPAR, _PRE = _trellis()
_SU = np.array([1.0, -1.0])


class _Audit:
    """Running, per block: is every finite value seen a multiple of the block's
    q, and the largest |value| / q.  Every array seen is [n][...]."""

    def __init__(self, q):
        self.q, self.exact, self.ratio = q, np.ones(len(q), dtype=bool), np.zeros(len(q))

    def see(self, x):
        x = np.asarray(x)
        v = x.reshape(len(self.q), -1) / self.q[:, None]             # q is a power of two: the division is exact
        fin = np.isfinite(v)
        self.exact &= (~fin | (v == np.rint(v))).all(axis=1)
        self.ratio = np.maximum(self.ratio, np.where(fin, np.abs(v), 0.0).max(axis=1))


def _bcjr_audited(ls, lp, la, aud):
    """One max-log BCJR pass over [n][steps] arrays; a-posteriori L [n][steps].
    (Inside, the step axis comes first so that a step's values are contiguous.)"""
    n, T = ls.shape
    G = (0.5 * ls.T)[:, :, None, None] * _SFB + (0.5 * lp.T)[:, :, None, None] * _SPAR + \
        (0.5 * la.T)[:, :, None, None] * _SU                            # [T][n][s][u], halves: exact products
    G0, G1 = np.ascontiguousarray(G[..., 0]), np.ascontiguousarray(G[..., 1])
    alpha = np.full((T + 1, n, 8), -np.inf)
    beta = np.full((T + 1, n, 8), -np.inf)
    alpha[0, :, 0] = 0.0
    beta[T, :, 0] = 0.0
    (pa, ua), (pb, ub) = (_PRE[:, 0] // 2, _PRE[:, 0] % 2), (_PRE[:, 1] // 2, _PRE[:, 1] % 2)
    Ga, Gb = G[:, :, pa, ua], G[:, :, pb, ub]                           # the two branches into each state
    n0, n1 = _NS[:, 0], _NS[:, 1]
    for k in range(T):
        a = alpha[k]
        np.maximum(a[:, pa] + Ga[k], a[:, pb] + Gb[k], out=alpha[k + 1])
    for k in range(T - 1, -1, -1):
        b = beta[k + 1]
        np.maximum(b[:, n0] + G0[k], b[:, n1] + G1[k], out=beta[k])
    L = ((alpha[:T] + G0) + beta[1:][:, :, n0]).max(axis=2) - ((alpha[:T] + G1) + beta[1:][:, :, n1]).max(axis=2)
    aud.see(G.transpose(1, 0, 2, 3))
    with np.errstate(invalid='ignore'):
        aud.see((alpha - alpha[:, :, :1]).transpose(1, 0, 2))
        aud.see((beta - beta[:, :, :1]).transpose(1, 0, 2))
    L = np.ascontiguousarray(L.T)
    aud.see(L)
    return L


Audit = collections.namedtuple('Audit', 'q exact ratio D')


def exactness_audit(O, llr, K, iters, scale=1.0, step=None):
    """The premise of the exact tie, checked on llr [3K + 12] or [n][3K + 12].
    Returns Audit(q, exact, ratio, D):
      q      the quantum: step / 2 for the metrics (gamma sums halves), halved
             once more per scaled half-iteration (scale = 0.5); step defaults
             to the largest power of two that divides every LLR, and may be
             given per block ([n]: blocks of several grids in one call; q is
             then [n] too, exact and ratio still the worst over the blocks)
      exact  whether every gamma, extrinsic, L and every finite alpha_s -
             alpha_0 and beta_s - beta_0 is an integer multiple of q
      ratio  the largest such magnitude / q; the premise holds below 2^22
      D      the decisions D(0) .. D(iters) [n][iters + 1][K] of this evaluation"""
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    n = len(llr)
    if step is None:
        nz = np.abs(llr[llr != 0])
        step = 1.0 if len(nz) == 0 else float(2.0 ** int(np.min(_low_bit_exp(nz))))
    halvings = 0 if scale == 1.0 else 2 * iters
    assert scale in (1.0, 0.5), 'only powers of two keep the grid'
    q = np.asarray(step, dtype=np.float64) / 2 / 2.0 ** halvings
    perm = O.qpp_perm(K)
    z3 = np.zeros((n, 3))
    body = llr[:, :3 * K].reshape(n, K, 3)
    sy, p1, p2 = body[:, :, 0], body[:, :, 1], body[:, :, 2]
    ls1 = np.concatenate([sy, llr[:, 3 * K:3 * K + 3]], axis=1)
    lp1 = np.concatenate([p1, llr[:, 3 * K + 3:3 * K + 6]], axis=1)
    ls2 = np.concatenate([sy[:, perm], llr[:, 3 * K + 6:3 * K + 9]], axis=1)
    lp2 = np.concatenate([p2, llr[:, 3 * K + 9:3 * K + 12]], axis=1)
    aud = _Audit(np.broadcast_to(q, (n,)))
    e21 = np.zeros((n, K))
    D = np.zeros((n, iters + 1, K), dtype=np.uint8)
    for it in range(iters + 1):
        la = np.concatenate([e21, z3], axis=1)
        app = _bcjr_audited(ls1, lp1, la, aud)
        D[:, it] = app[:, :K] < 0
        if it == iters:
            break
        e12 = scale * ((app - la) - ls1)[:, :K]
        aud.see(e12)
        la = np.concatenate([e12[:, perm], z3], axis=1)
        e = scale * ((_bcjr_audited(ls2, lp2, la, aud) - la) - ls2)[:, :K]
        aud.see(e)
        e21 = np.zeros((n, K))
        e21[:, perm] = e
    return Audit(q if q.ndim else float(q), bool(aud.exact.all()), float(aud.ratio.max()), D)


def _low_bit_exp(x):
    """Exponent of the lowest set bit of each float64 in x (x != 0)."""
    m, e = np.frexp(x)                       # x = m 2^e, 0.5 <= |m| < 1
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return e - 53 + np.log2(low.astype(np.float64)).astype(np.int64)


# ---------------------------------------------------------------------------
# The reference's answers, once per pool block
def reference(O, K, quant):
    """D [n][ITERS + 1][K]: D[b][n] = oracle.turbo_decode(llr[b], K, n).  One
    pass of the restated loop (turbo_scaled_model.decisions_f64, scale 1) gives
    all nine; the fixed decoders' iteration counts 1, 2 and 8 are the
    oracle's own turbo_decode and are asserted equal to that loop here."""
    key = (K, quant, SEED[(K, quant)])
    if key not in _REF:
        p = quant_pool(O, K, quant)
        D = np.array([M.decisions_f64(O, l, K, ITERS) for l in p.llr])
        for b, l in enumerate(p.llr):
            for n in (1, 2, ITERS):
                assert np.array_equal(D[b, n], O.turbo_decode(l, K, n)), (K, quant, b, n)
        _REF[key] = D
    return _REF[key]


def reference_scaled(O, K, quant):
    """D [n][SC_ITERS + 1][K] of the float64 model at scale 0.5."""
    key = (K, quant, SEED[(K, quant)])
    if key not in _SC:
        p = quant_pool(O, K, quant)
        _SC[key] = np.array([M.decisions_f64(O, l, K, SC_ITERS, SC_SCALE) for l in p.llr])
    return _SC[key]


def final_app(O, llr, K, iters=ITERS):
    """The reference's a-posteriori L [K] of the pass that ends a decode of
    `iters` iterations: its decoder-1 pass on the last extrinsic of the trace."""
    _, tr = O.turbo_decode(llr, K, iters, trace=True)
    la = np.concatenate([tr[iters - 1], np.zeros(3)])
    return O.bcjr_app(np.concatenate([llr[0:3 * K:3], llr[3 * K:3 * K + 3]]),
                      np.concatenate([llr[1:3 * K:3], llr[3 * K + 3:3 * K + 6]]), la)[:K]


def rules(O, D, crc, iters=None):
    """(n* [n], passed [n]) of the early-stop rule on precomputed D [n][iters + 1][K]."""
    iters = D.shape[1] - 1 if iters is None else iters
    res = [M.rule(O, None, D.shape[2], iters, POLYS[crc], D=d) for d in D]
    return np.array([r[1] for r in res]), np.array([r[2] for r in res])


def lanes(O, K, quant):
    """Pool index of each of the NCB lanes: wave 0 cycles the whole pool; wave 1
    holds the known-answer blocks interleaved with blocks the reference fails,
    so that a degenerate lane's neighbours are live, undecided lanes; the
    partial wave holds a decoded, a failed and a known-answer block."""
    p = quant_pool(O, K, quant)
    D = reference(O, K, quant)
    n = len(p.kind)
    ka = np.flatnonzero(p.kind != 0)
    ok = (D[:, ITERS] == p.sent).all(axis=1)
    fail = np.flatnonzero((p.kind == 0) & ~ok)
    good = np.flatnonzero((p.kind == 0) & ok)
    w1 = np.empty(64, dtype=np.int64)
    w1[0::2] = ka[np.arange(32) % len(ka)]
    w1[1::2] = fail[np.arange(32) % len(fail)]
    return np.concatenate([np.arange(64) % n, w1, [good[0], fail[-1], ka[1]]])


def ties(O, K):
    """[(block, positions)] of the step-1.0 pool's ladder blocks whose reference
    L after ITERS iterations is exactly 0 somewhere."""
    key = (K, SEED[(K, 's1')])
    if key not in _TIES:
        p = quant_pool(O, K, 's1')
        out = []
        for b in np.flatnonzero(p.kind == 0):
            z = np.flatnonzero(final_app(O, p.llr[b], K) == 0.0)
            if len(z):
                out.append((int(b), z))
        _TIES[key] = out
    return _TIES[key]


def pool_conditions(O, K):
    """The figures of the conditions, per K:
      'decoded' / 'failed'   per quantisation, the fraction of ladder blocks the reference decodes / fails
      'ties'                 positions with reference L == 0 after ITERS iterations, step-1.0 ladder blocks
      'ties_that_matter'     of those, the ones in a block the reference otherwise decodes or at a sent 1
      'n_star'               per quantisation and generator, the distinct n* of wave 0 and whether one never passes"""
    out = {'decoded': {}, 'failed': {}, 'n_star': {}}
    for quant in QUANT:
        p, D = quant_pool(O, K, quant), reference(O, K, quant)
        lad = p.kind == 0
        ok = (D[:, ITERS] == p.sent).all(axis=1)
        out['decoded'][quant] = float(np.mean(ok[lad]))
        out['failed'][quant] = float(np.mean(~ok[lad]))
        w0 = lanes(O, K, quant)[:64]
        for crc in POLYS:
            n_star, passed = rules(O, D, crc)
            out['n_star'][(quant, crc)] = (sorted(set(n_star[w0][passed[w0]].tolist())), bool((~passed[w0]).any()))
    p, D = quant_pool(O, K, 's1'), reference(O, K, 's1')
    tz = ties(O, K)
    out['ties'] = int(sum(len(z) for _, z in tz))
    matter = 0
    for b, z in tz:
        rest = np.ones(K, dtype=bool)
        rest[z] = False
        decodes = bool((D[b, ITERS] == p.sent[b])[rest].all())
        matter += len(z) if decodes else int(p.sent[b][z].sum())
    out['ties_that_matter'] = matter
    return out


def assert_pool_conditions(O, K):
    """Conditions, not measurements: move SEED, never these."""
    c = pool_conditions(O, K)
    for quant in QUANT:
        assert c['decoded'][quant] >= 0.25 and c['failed'][quant] >= 0.25, (K, quant, c['decoded'], c['failed'])
        for crc in POLYS:
            stops, never = c['n_star'][(quant, crc)]
            assert never and len(stops) + 1 >= 3, (K, quant, crc, stops, never)     # the `mixing` condition
    assert c['ties'] >= 8, (K, c['ties'])
    assert c['ties_that_matter'] >= 1, (K, c['ties'])
    return c


# ---------------------------------------------------------------------------
# What the known-answer blocks must decode to, from their construction alone
def known_answer(p, b, n):
    """The decisions [K] of pool block b after n iterations where they follow
    without a decoder, else None.
      ZERO    every metric ties, every L is exactly 0.0, and 0.0 < 0 is false: all zeros.
      NOPAR   n = 0 only.  The reference's "systematic" stream is the feedback
              bit a_k (turbo_encoder.py:137-211), so with the parities erased
              the path metric is sum_k +-Ls_k / 2 over a free sequence a, and
              u_k = a_k ^ a_(k-2) ^ a_(k-3).  Flipping u_k costs the cheapest of
              those a: L_k = prod sign(Ls_j) min |Ls_j| over j in {k, k-2, k-3},
              j >= 0 -- exactly 0, so decision 0, if one of them is 0.0.  (The
              extrinsic L - Ls of that pass is not zero, so later iterations
              are not constraint-free; they are compared with the reference
              like any other block.)
      CLIP_*  every n: the sent word (the *_NOSYS ones from the parities alone)."""
    kind = p.kind[b]
    K = p.sent.shape[1]
    if kind == ZERO:
        return np.zeros(K, dtype=np.uint8)
    if kind == NOPAR:
        if n != 0:
            return None
        ls = p.llr[b][0:3 * K:3]
        neg, zero = (ls < 0).astype(np.uint8), ls == 0
        out = neg.copy()
        for back in (2, 3):
            out[back:] ^= neg[:-back]
            zero = zero | np.concatenate([np.zeros(back, dtype=bool), (ls == 0)[:-back]])
        out[zero] = 0
        return out
    if kind in (CLIP_A, CLIP_A_NOSYS, CLIP_B, CLIP_B_NOSYS):
        return p.sent[b]
    return None


def known_n_star(p, b, crc):
    """n* of pool block b under generator `crc` where it follows without a
    decoder (1: the all-zero word passes the zero-init CRC, a clipped block
    decodes at once and carries its own generator's CRC), else None."""
    if p.kind[b] == ZERO or (p.kind[b] in (CLIP_A, CLIP_A_NOSYS, CLIP_B, CLIP_B_NOSYS) and p.crc[b] == crc):
        return 1
    return None


# ---------------------------------------------------------------------------
# Scale invariance: unquantised Gaussian LLRs through float32
def gaussian_blocks(O, K, n, seed=0):
    """n blocks (payload + CRC-24B) on a ladder across the cliff of K: (llr
    [n][3K + 12] float64 holding float32 values, sent [n][K])."""
    rs = np.random.RandomState(7919 * seed + K)
    lo, hi, _ = LADDER[K]
    llr, sent = [], []
    for snr in np.linspace(lo, hi, n):
        pay = rs.randint(0, 2, K - 24).astype(np.uint8)
        cb = np.concatenate([pay, O.crc_bits(pay, POLYS['24B'], 24)])
        s2 = 10 ** (-snr / 10)
        y = 1 - 2.0 * O.turbo_encode(cb) + np.sqrt(s2) * rs.randn(3 * K + 12)
        llr.append((2 * y / s2).astype(np.float32).astype(np.float64))
        sent.append(cb)
    return np.array(llr), np.array(sent)
