"""The coded TM4 chain (LTE_CHAIN_SPATIAL_CODED, include/lte_phy.h) modelled from
the oracle's primitives (a helper of tests/test_spatial_coded_host.py and
tests/test_gpu_spatial_coded.py, not a conftest).

The definition: simulate_siso_coded's coding chain around
simulate_spatial_multiplexing's transmitter, link and per-symbol CRS estimate.
Everything here is lte_oracle's CRC / segment / turbo_encode / rate_match /
bits_to_symbols / tf_interleave_perm / pilots / llrs / coded_rx_decode,
mimo_oracle's layer_map / mimo_pilot_indices / _ofdm_time / transmit_sm /
_fft_symbols / mimo_estimate and tm4_oracle.codebook, plus the one rule that is
this chain's own, evaluated with np.linalg.inv (soft_rule):
  MMSE  A = He^H He + s2 I, s = A^-1 He^H y, e_l = s2 (A^-1)_ll,
        mu_l = max(1 - e_l, 1e-6), z_l = s_l / mu_l, nv_l = e_l / mu_l
  ZF    A = He^H He, z = s, nv_l = s2 min((A^-1)_ll, 1e6)
  MRC   z = conj(h) y / ||h||^2, nv = s2 min(1 / ||h||^2, 1e6)
with s2 = 10^(-SNR/10).  Per subcarrier it also returns kappa = cond(A) and
mu_min = min_l mu_l (1 for ZF / MRC): the scale of the tolerances."""
import numpy as np

FRAMES = 64 + 3          # one full 64-frame decoder group and a partial one
ITERS = 2
MIN_PASS = MIN_FAIL = 8
PMI = 0

# r_cpu: the worst disagreement of two float64 evaluations of the soft rule
# (soft_rule's np.linalg.inv and soft_rule_chol's Cholesky / L^-1 / diagonal, the
# kernel's order) over every subcarrier of the ladder below, in units of
# 2^-52 kappa / mu_min times ||z|| (z) or (1 + |LLR|) (LLRs).  Measured 2718.757
# (case C44, an LLR: at 36 dB a 64-QAM LLR moves by 1 / nv ~ 4e3 per unit of z;
# P22 109, R44 483, R43 328, Z42 278, D22 1257, M21 0: both evaluate MRC alike) by
#   python -m pytest tests/test_spatial_coded_host.py -k tolerance -s
# which prints the value per case and holds this constant to it.
R_CPU = 2719.0

# The ladder: numerology, channel, TB size, antennas / rank / detector and the SNR
# window (dB) whose linspace over the 67 frames straddles the turbo cliff at 2
# iterations.  The last subcarrier is partly filled (Nd no multiple of the rank) in
# R44, Z42, D22 and C44 (R43's Nd = 249 = 3 * 83 is a multiple); D22: N = 1024.
CASES = {
    'P22': dict(bw=1.25, mod='QPSK', chan='awgn', prof='Pedestrian_A', n_bits=435, ntx=2, nrx=2, rank=2, det='MMSE',
                snr=(0.0, 25.0)),
    'M21': dict(bw=1.25, mod='QPSK', chan='awgn', prof='Pedestrian_A', n_bits=435, ntx=2, nrx=2, rank=1, det='MRC',
                snr=(-6.0, 10.0)),
    'R44': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=2041, ntx=4, nrx=4, rank=4,
                det='MMSE', snr=(8.0, 30.0)),
    'R43': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=2041, ntx=4, nrx=4, rank=3,
                det='MMSE', snr=(4.0, 24.0)),
    'Z42': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=2041, ntx=4, nrx=3, rank=2,
                det='ZF', snr=(2.0, 20.0)),
    'D22': dict(bw=10.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=2041, ntx=2, nrx=2, rank=2,
                det='MMSE', snr=(6.0, 30.0)),
    'C44': dict(bw=20.0, mod='64-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=6121, ntx=4, nrx=4, rank=4,
                det='MMSE', snr=(14.0, 36.0)),
}


def numerology(O, cs):
    return O.Numerology(bandwidth=cs['bw'], modulation=cs['mod'])


def precoder(T, cs, pmi=PMI):
    return np.asarray(T.codebook(cs['ntx'], 'TM4', cs['rank'])[pmi], dtype=complex)


def n_paths(O, num, cs):
    return len(O.itu_paths(num, cs['prof'], spatial=True)[0]) if cs['chan'] == 'rayleigh_mp' else 0


def deinterleave_index(n_coded_syms, Nd):
    """src with coded symbol q = RE src[q] of the grid (the T/F interleaver of
    the coded chain: rows of Nd written, columns read)."""
    rows = -(-n_coded_syms // Nd)
    q = np.arange(n_coded_syms)
    return (q % Nd) * rows + q // Nd


def transmit(O, MO, num, cs, bits, W):
    """LTE_CHAIN_CODED's coding, then LTE_CHAIN_SPATIAL's transmitter per OFDM
    symbol on the Nd interleaved QAM symbols (padding symbols are zeros)."""
    tbc = O.attach_crc24a(np.asarray(bits).astype(np.int64))
    cbs, plan = O.segment(tbc)
    rms = []
    for cb in cbs:
        enc = O.turbo_encode(cb)
        rms.append(O.rate_match(enc, len(enc), len(cb), 0))
    coded = np.concatenate(rms)
    qam = O.bits_to_symbols(coded, num.modulation)
    perm, rows, total = O.tf_interleave_perm(len(qam), num.Nd)
    inter = np.pad(qam, (0, total - len(qam)))[perm]
    ntx, rank = cs['ntx'], cs['rank']
    pidx = MO.mimo_pilot_indices(num, ntx)
    sig = [[] for _ in range(ntx)]
    for i in range(rows):
        lay = MO.layer_map(inter[i * num.Nd:(i + 1) * num.Nd], rank)
        grids = np.zeros((ntx, num.N), dtype=complex)
        for di in range(lay.shape[1]):
            grids[:, num.data_idx[di]] = W @ lay[:, di]
        for t in range(ntx):
            grids[t, pidx[t]] = O.pilots(t % 4, len(pidx[t]))
            sig[t].append(MO._ofdm_time(num, grids[t]))
    return dict(xs=[np.concatenate(s) for s in sig], coded=coded, plan=plan, rm_lens=[len(r) for r in rms],
                n_sym=rows)


def soft_rule(He, y, s2, det):
    """The chain's soft-output rule on stacked subcarriers He [n][rx][R], y [n][rx]
    with np.linalg.inv -> z [n][R], nv [n][R], kappa [n], mu_min [n]."""
    n, _, R = He.shape
    Hh = np.conj(np.swapaxes(He, 1, 2))
    G = Hh @ He
    rhs = (Hh @ y[:, :, None])[:, :, 0]
    if det == 'MRC':
        n2 = np.real(G[:, 0, 0])
        return rhs / n2[:, None], s2 * np.minimum(1.0 / n2, 1e6)[:, None], np.ones(n), np.ones(n)
    A = G if det == 'ZF' else G + s2 * np.eye(R)
    Ai = np.linalg.inv(A)
    s = (Ai @ rhs[:, :, None])[:, :, 0]
    q = np.real(np.diagonal(Ai, axis1=1, axis2=2))
    kappa = np.linalg.cond(A)
    if det == 'ZF':
        return s, s2 * np.minimum(q, 1e6), kappa, np.ones(n)
    e = s2 * q
    mu = np.maximum(1.0 - e, 1e-6)
    return s / mu, e / mu, kappa, mu.min(axis=1)


def soft_rule_chol(He, y, s2, det, raw=False):
    """The same rule in the kernel's order: Cholesky A = L L^H, the triangular
    inverse L^-1 by forward substitution, s = L^-H (L^-1 rhs), (A^-1)_ll =
    sum_k |(L^-1)_kl|^2 -> z, nv.  raw: the hard-output detectors' s instead
    (MMSE: before the division by mu; ZF and MRC: z itself)."""
    n, _, R = He.shape
    Hh = np.conj(np.swapaxes(He, 1, 2))
    G = Hh @ He
    rhs = (Hh @ y[:, :, None])[:, :, 0]
    if det == 'MRC':
        n2 = np.real(G[:, 0, 0])
        if raw:
            return rhs / n2[:, None]
        return rhs / n2[:, None], s2 * np.minimum(1.0 / n2, 1e6)[:, None]
    A = G if det == 'ZF' else G + s2 * np.eye(R)
    L = np.linalg.cholesky(A)
    Li = np.zeros_like(L)
    for k in range(R):
        Li[:, k, k] = 1.0 / np.real(L[:, k, k])
        for i in range(k + 1, R):
            v = np.zeros(n, dtype=complex)
            for j in range(k, i):
                v = v - L[:, i, j] * Li[:, j, k]
            Li[:, i, k] = v / np.real(L[:, i, i])
    u = (Li @ rhs[:, :, None])[:, :, 0]
    s = (np.conj(np.swapaxes(Li, 1, 2)) @ u[:, :, None])[:, :, 0]
    if raw:
        return s
    q = np.sum(np.abs(Li) ** 2, axis=1)
    if det == 'ZF':
        return s, s2 * np.minimum(q, 1e6)
    e = s2 * q
    mu = np.maximum(1.0 - e, 1e-6)
    return s / mu, e / mu


def receive(O, MO, num, cs, ys, n_sym, W, snr_db, rule=soft_rule):
    """FFT, per-symbol CRS estimate, H_eff = H W and the soft rule per data
    subcarrier.  In RE order (layer t of subcarrier j is RE R j + t of the symbol,
    dropped past Nd) [n_sym * Nd]: z, nv, kappa, mu_min, and ||z|| of the RE's
    subcarrier; He / y [n_sym * n_dsc] are kept for the second evaluation."""
    ntx, nrx, rank, Nd = cs['ntx'], cs['nrx'], cs['rank'], num.Nd
    n_dsc = -(-Nd // rank)
    s2 = 10 ** (-snr_db / 10)
    per_rx = [MO._fft_symbols(num, ys[r], n_sym) for r in range(nrx)]
    sc = num.data_idx[:n_dsc]
    Hes, yv = [], []
    for i in range(n_sym):
        g = np.array([per_rx[r][i] for r in range(nrx)])
        H = MO.mimo_estimate(num, g, ntx)                       # [rx][tx][N]
        Hes.append(np.stack([H[:, :, k] @ W for k in sc]))       # [n_dsc][rx][R]
        yv.append(g[:, sc].T)
    He, y = np.concatenate(Hes), np.concatenate(yv)
    out = rule(He, y, s2, cs['det'])
    res = dict(He=He, y=y)
    z = out[0]
    zn = np.linalg.norm(z, axis=1)
    per = dict(z=z, nv=out[1])
    if len(out) == 4:
        per.update(kappa=np.repeat(out[2][:, None], rank, 1), mu_min=np.repeat(out[3][:, None], rank, 1),
                   z_norm=np.repeat(zn[:, None], rank, 1))
    for k, v in per.items():                                     # [n_sym * n_dsc][R] -> RE order, cut at Nd
        res[k] = v.reshape(n_sym, n_dsc * rank)[:, :Nd].reshape(-1)
    return res


def llrs_re(O, num, z, nv):
    """Max-log LLRs in RE order [n_re * bps]."""
    return O.llrs(z, nv, num.modulation)


def decode_llrs(O, num, seg, coded_len, llr_re, iters=ITERS, f32=False):
    """The oracle's RX decode of an LLR array in RE order [n_re * bps]: T/F
    de-interleave, dematch, turbo, desegmentation, CRC-24A -> (bits, crc)."""
    src = deinterleave_index(coded_len // num.bps, num.Nd)
    L = np.asarray(llr_re, dtype=np.float64).reshape(-1, num.bps)[src].reshape(-1)[:coded_len]
    return O.coded_rx_decode(L.astype(np.float32) if f32 else L, seg, [3 * p[0] + 12 for p in seg], iters,
                             f32_model=f32)


def frame(O, MO, T, num, cs, bits, snr_db, draws, fD=0.0, iters=ITERS, pmi=PMI):
    """One frame through the model.  draws: mimo_oracle.transmit_sm's format."""
    bits = np.asarray(bits).astype(np.int64)
    W = precoder(T, cs, pmi)
    tx = transmit(O, MO, num, cs, bits, W)
    ys, Hm = MO.transmit_sm(num, tx['xs'], cs['nrx'], cs['chan'], snr_db, cs['prof'], fD, draws)
    rx = receive(O, MO, num, cs, ys, tx['n_sym'], W, snr_db)
    llr = llrs_re(O, num, rx['z'], rx['nv'])
    dec, ok = decode_llrs(O, num, tx['plan'], len(tx['coded']), llr, iters)
    dec = np.asarray(dec)[:len(bits)]
    return dict(tx=tx, rx=rx, z=rx['z'], nv=rx['nv'], llr=llr, bits_rx=dec, crc=bool(ok),
                errs=int(np.sum(bits != dec)), channel_matrix=Hm, W=W)


def frame_len(O, MO, T, num, cs):
    """Samples per TX stream of the case's frame."""
    return len(transmit(O, MO, num, cs, np.zeros(cs['n_bits'], dtype=np.int64), precoder(T, cs))['xs'][0])


def case_inputs(O, MO, T, name, frames=FRAMES):
    """Frame f from RandomState(n_bits + f): randint bits first, then
    transmit_sm_draws from the same stream (set as the global state for the
    call).  Also the injection arrays of lte_run: phases [F][rx][tx][P][16],
    link_h [F][rx][tx][2], noise [F][rx][2][L].  name: a ladder case, or a case
    dict of the same keys."""
    cs = CASES[name] if isinstance(name, str) else name
    num = numerology(O, cs)
    L = frame_len(O, MO, T, num, cs)
    P = n_paths(O, num, cs)
    ntx, nrx = cs['ntx'], cs['nrx']
    bits = np.zeros((frames, cs['n_bits']), dtype=np.uint8)
    ph = np.zeros((frames, nrx, ntx, max(P, 1), 16))
    lh = np.zeros((frames, nrx, ntx, 2))
    z = np.zeros((frames, nrx, 2, L))
    draws = []
    saved = np.random.get_state()
    try:
        for f in range(frames):
            rs = np.random.RandomState(cs['n_bits'] + f)
            bits[f] = rs.randint(0, 2, cs['n_bits'])
            np.random.set_state(rs.get_state())
            d = MO.transmit_sm_draws(ntx, nrx, cs['chan'], L, cs['prof'])
            draws.append(d)
            for r in range(nrx):
                for t in range(ntx):
                    lk = d['links'][r][t]
                    if P:
                        ph[f, r, t] = np.stack(lk['phases'])
                    else:
                        lh[f, r, t] = lk['h'].real, lk['h'].imag
                z[f, r, 0], z[f, r, 1] = d['noise'][r]['z_re'], d['noise'][r]['z_im']
    finally:
        np.random.set_state(saved)
    return dict(bits=bits, ph=ph, lh=lh, z=z, draws=draws, snrs=np.linspace(cs['snr'][0], cs['snr'][1], frames),
                L=L, P=P)


def early_stop_n_star(O, L, seg, iters):
    """CRC early termination evaluated by the oracle on LLRs in coded order: per
    code block the first iteration n* in 1..iters whose decisions pass the
    block's CRC-24 (24A for a single block, else 24B), `iters` if none does."""
    poly = O.CRC24A_POLY if len(seg) == 1 else O.CRC24B_POLY
    off, out = 0, []
    for K, F, info, o, crc in seg:
        dm = O.rate_dematch(L[off:off + 3 * K + 12], K, 0)
        off += 3 * K + 12
        n_star = iters
        for n in range(1, iters + 1):
            if not O.crc_bits(O.turbo_decode(dm, K, n), poly, 24).any():
                n_star = n
                break
        out.append(n_star)
    return out


def philox_frame(O, MO, T, P, num, cs, seed, frame_id, snr_db, fD=0.0, iters=ITERS):
    """One run_grid frame: the frame's Philox payload and LTE_CHAIN_SPATIAL's
    streams (philox.sm_draws) through the model."""
    bits = P.payload_bits(seed, frame_id, cs['n_bits'])
    L = frame_len(O, MO, T, num, cs)
    d = P.sm_draws(seed, frame_id, L, cs['ntx'], cs['nrx'], cs['chan'], n_paths(O, num, cs))
    return frame(O, MO, T, num, cs, bits, snr_db, d, fD=fD, iters=iters)


_CACHE = {}


def case_frames(O, MO, T, name):
    """The model's 67 frames of a ladder case on case_inputs (computed once,
    velocity 0)."""
    if name not in _CACHE:
        cs = CASES[name]
        num = numerology(O, cs)
        inp = case_inputs(O, MO, T, name)
        _CACHE[name] = (inp, [frame(O, MO, T, num, cs, inp['bits'][f], float(inp['snrs'][f]), inp['draws'][f])
                              for f in range(FRAMES)])
    return _CACHE[name]


def tolerance_ratio(O, MO, T, name):
    """The worst disagreement of soft_rule and soft_rule_chol over the case's
    subcarriers, scaled as R_CPU is (the module docstring)."""
    cs = CASES[name]
    num = numerology(O, cs)
    inp, frames = case_frames(O, MO, T, name)
    worst = 0.0
    eps = 2.0 ** -52
    n_dsc = -(-num.Nd // cs['rank'])
    for f, fr in enumerate(frames):
        rx = fr['rx']
        z2, nv2 = soft_rule_chol(rx['He'], rx['y'], 10 ** (-float(inp['snrs'][f]) / 10), cs['det'])
        n_sym = fr['tx']['n_sym']
        z2, nv2 = (v.reshape(n_sym, n_dsc * cs['rank'])[:, :num.Nd].reshape(-1) for v in (z2, nv2))
        scale = eps * rx['kappa'] / rx['mu_min']
        worst = max(worst, float(np.max(np.abs(z2 - rx['z']) / (scale * rx['z_norm']))))
        l1, l2 = fr['llr'], llrs_re(O, num, z2, nv2)
        worst = max(worst, float(np.max(np.abs(l2 - l1) / (np.repeat(scale, num.bps) * (1 + np.abs(l1))))))
    return worst
