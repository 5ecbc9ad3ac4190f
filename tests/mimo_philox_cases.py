"""The cases of tests/test_gpu_mimo_philox.py and their oracle side (a helper of
that file and of tests/test_oracle_mimo_philox.py, not a conftest).

Every case is B = 5 frames with the frame ids IDS on the device's own Philox
draws: the payload (philox.payload_bits) and the chain's streams
(philox.sfbc_draws / sm_draws / bf_draws / siso_draws) of (seed, id) through
the float64 oracle.  Nothing here needs a GPU: the preconditions of the GPU
file's exact comparisons (decision-boundary margins, the mix of clean and
broken frames) are evaluated from the oracle alone.

seed: chosen on the CPU, the first of 1, 2, 3, ... for which the case's
preconditions hold for every RE of every frame (no RE is exempted): 1 for
every case but sfbc_vb5_u (403) and sfbc_pb20_c (549), whose channels the
reference's receiver follows only in a rare frame (frame_mix_ok).
"""
import numpy as np

from oracle import bf_oracle as BF
from oracle import lte_oracle as O
from oracle import mimo_oracle as MO
from oracle import philox as P
from oracle import tm4_oracle as T

import spatial_coded_model as SCM

B = 5
IDS = np.array([0, 1, 2, 2 ** 32 + 3, 65535], dtype=np.uint64)   # 2^32 + 3: the counter's frame_hi word
BOUNDARY_MARGIN = 1e-9      # of the constellation spacing (tests/test_gpu_profiles.py)
TB = 2041                   # coded cases: one code block, K = 2112
ITERS = 2
NEARLY_CLEAN = 1e-2         # an uncoded frame with a BER below this counts as nearly clean
EPS = 2.0 ** -52

# r of the spatial cases' margin m_k = max(1e-9, r eps kappa_k / mu_k): the worst
# disagreement, over every subcarrier of every SM_CASES frame, of two float64
# evaluations of the detector on the CPU -- the oracle's (np.linalg.inv / pinv,
# tm4_oracle.detect) and the kernel's Cholesky order
# (spatial_coded_model.soft_rule_chol(raw=True)) -- in units of eps kappa / mu_min
# ||s|| (as spatial_coded_model.R_CPU).  Measured by
#   python -m pytest tests/test_oracle_mimo_philox.py -k spatial_r -s
# which prints the value per case and holds this constant to it.  Measured 13.918
# (sm_42_r1_mrc: kappa = mu = 1 there, and the reference's dot(conj(h) / ||h||^2, y)
# against (h^H y) / ||h||^2; sm_r3_zf 3.58, the MMSE / SIC cases 0.55 to 1.83).
R_SPATIAL = 14.0

_QS = {'QPSK': np.sqrt(2.0), '16-QAM': np.sqrt(10.0), '64-QAM': np.sqrt(42.0)}
_NL = {'QPSK': 2, '16-QAM': 4, '64-QAM': 8}
_G9 = (1.0, 0.95, 0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6)
SNRS = (0.0, 7.5, 15.0, 22.5, 30.0)


def boundary_distances(syms, mod):
    """Per symbol, the smallest distance of its real or imaginary part to a
    decision boundary of the square constellation, in units of its spacing."""
    nl, sc = _NL[mod], _QS[mod]
    bnd = (np.arange(1, nl) * 2 - nl) / sc
    syms = np.asarray(syms).reshape(-1)
    d = np.minimum(np.min(np.abs(syms.real[:, None] - bnd[None, :]), axis=1),
                   np.min(np.abs(syms.imag[:, None] - bnd[None, :]), axis=1))
    return d / (2.0 / sc)


def numerology(cs):
    return O.Numerology(bandwidth=cs['bw'], modulation=cs['mod'], cp_type=cs.get('cp', 'normal'))


# ---------------------------------------------------------------------------
# Beamforming: every antenna shape in both update modes.  1 / num_rx of the MRT
# mean is exact for 1, 2, 4, 8 RX only (3 and 5: where k_bf_setup's reciprocal can
# differ from np.mean's division).  bf_21*: 1.25 MHz, 3 symbols: 5 * 3 * 62 = 930
# REs, no multiple of 256 (k_bf_data's tail lanes run); bf_88*: 20 MHz.
def _bf(bw, mod, ntx, nrx, mode, seed=1, n_sym=3, snrs=(-4.0, 2.0, 8.0, 16.0, 26.0)):
    return dict(bw=bw, mod=mod, ntx=ntx, nrx=nrx, mode=mode, seed=seed, n_sym=n_sym, snrs=snrs)


BF_CASES = {
    'bf_21a': _bf(1.25, 'QPSK', 2, 1, 'adaptive'), 'bf_21s': _bf(1.25, '16-QAM', 2, 1, 'static'),
    'bf_41a': _bf(5.0, '16-QAM', 4, 1, 'adaptive'), 'bf_41s': _bf(5.0, '64-QAM', 4, 1, 'static'),
    'bf_81a': _bf(5.0, '64-QAM', 8, 1, 'adaptive'), 'bf_81s': _bf(5.0, 'QPSK', 8, 1, 'static'),
    'bf_24a': _bf(5.0, '64-QAM', 2, 4, 'adaptive'), 'bf_24s': _bf(5.0, '16-QAM', 2, 4, 'static'),
    'bf_43a': _bf(5.0, '16-QAM', 4, 3, 'adaptive'), 'bf_43s': _bf(5.0, '64-QAM', 4, 3, 'static'),
    'bf_85a': _bf(5.0, '64-QAM', 8, 5, 'adaptive'), 'bf_85s': _bf(5.0, '16-QAM', 8, 5, 'static'),
    'bf_88a': _bf(20.0, '16-QAM', 8, 8, 'adaptive'), 'bf_88s': _bf(20.0, '64-QAM', 8, 8, 'static'),
}
PMI_MARGIN = 1e-9    # relative gap between the best and the second-best PMI metric ||H w||^2


def uncoded_bits(num, n_sym, res=None):
    """Five bits short of the frame: the last RE is part payload, part padding."""
    return n_sym * (num.Nd if res is None else res) * num.bps - 5


def bf_frames(name, seed=None, snrs=None):
    cs = BF_CASES[name]
    num = numerology(cs)
    seed = cs['seed'] if seed is None else seed
    n_bits = uncoded_bits(num, cs['n_sym'])
    cb = T.codebook(cs['ntx'], 'TM6', 1)
    out = []
    for b, fid in enumerate(IDS):
        bits = P.payload_bits(seed, int(fid), n_bits).astype(np.int64)
        d = P.bf_draws(seed, int(fid), cs['ntx'], cs['nrx'], cs['n_sym'], num.Nd)
        snr = float((cs['snrs'] if snrs is None else snrs)[b])
        o = BF.simulate_beamforming(num, bits, snr, cs['ntx'], cs['nrx'], 'TM6', cs['mode'], draws=d)
        m = np.sort([np.sum(np.abs(d['H'] @ w) ** 2) for w in cb])
        out.append(dict(bits=bits, bits_rx=np.asarray(o['bits_received_array']).astype(np.uint8),
                        errs=int(o['bit_errors']), syms=o['symbols_rx'], H=o['channel_matrix'],
                        pmi=int(o['pmi_history'][0]), gain=float(o['beamforming_gain_db']),
                        margin=float(boundary_distances(o['symbols_rx'], cs['mod']).min()),
                        pmi_gap=float((m[-1] - m[-2]) / m[-1]), n_bits=n_bits))
    return out


# ---------------------------------------------------------------------------
# Uncoded SC-FDM (DFT-precoded SISO; the SIMO combiner has no de-precoder, as in
# the reference, so sc_simo's BER stays near 0.5 at every SNR: its frames all
# have errors and none is nearly clean -- the comparison is per frame all the same)
SC_CASES = {
    'sc_siso_pa5': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', nrx=1, n_sym=3, seed=1,
                        snrs=(5.0, 15.0, 25.0, 35.0, 45.0)),
    'sc_simo_flat125': dict(bw=1.25, mod='QPSK', chan='awgn', prof='Pedestrian_A', nrx=2, n_sym=3, seed=1,
                            snrs=SNRS),
}


def sc_frames(name, seed=None, snrs=None):
    cs = SC_CASES[name]
    num = numerology(cs)
    seed = cs['seed'] if seed is None else seed
    n_bits = uncoded_bits(num, cs['n_sym'])
    L = cs['n_sym'] * (num.N + num.cp)
    n_paths = len(O.itu_paths(num, cs['prof'])[0]) if cs['chan'] == 'rayleigh_mp' else 0
    out = []
    for b, fid in enumerate(IDS):
        bits = P.payload_bits(seed, int(fid), n_bits).astype(np.int64)
        d = P.siso_draws(seed, int(fid), L, n_paths, cs['nrx'])
        snr = float((cs['snrs'] if snrs is None else snrs)[b])
        if cs['nrx'] == 1:
            o = O.simulate_siso(num, bits, snr, cs['chan'], cs['prof'], 0.0, draws=d, sc_fdm=True)
            syms = o['symbols_rx']
        else:
            o = O.simulate_simo(num, bits, snr, cs['nrx'], cs['chan'], cs['prof'], 0.0, draws=d, sc_fdm=True)
            syms = o['symbols_rx_combined']
        # the scale of the symbols' tolerance (sc_sym_bound), from the receiver's inputs
        rxs = [o['signal_rx']] if cs['nrx'] == 1 else o['signal_rx_list']
        Yd = [O.demod_stream(num, y)[:, num.data_idx] for y in rxs]                          # [rx][sym][Nd]
        Hd = [np.stack(O.estimate_periodic(num, O.demod_stream(num, y))[0])[:, num.data_idx] for y in rxs]
        if cs['nrx'] == 1:     # ZF per RE max|Y| / |H|; the de-precoder is unitary: the L2 norm per OFDM symbol
            scale = np.max(np.abs(Yd[0])) * np.sqrt(np.sum(1.0 / np.abs(Hd[0]) ** 2, axis=1))
        else:                  # MRC per RE (no de-precoder in the SIMO combiner)
            scale = (np.sqrt(sum(np.max(np.abs(v)) ** 2 for v in Yd)) /
                     np.sqrt(sum(np.abs(h) ** 2 for h in Hd))).reshape(-1)
        out.append(dict(bits=bits, bits_rx=np.asarray(o['bits_received_array']).astype(np.uint8),
                        errs=int(o['bit_errors']), syms=syms, n_bits=n_bits, scale=scale,
                        margin=float(boundary_distances(syms, cs['mod']).min())))
    return out


# ---------------------------------------------------------------------------
# SFBC (2 TX Alamouti).  chan 'rayleigh_mp' with an ITU profile or a custom tap
# set (paths), or 'awgn' (flat links exp(j t pi / 2)).
def _sfbc(bw, mod, prof='Pedestrian_A', nrx=2, coded=False, n_sym=3, cp='normal', paths=None, chan='rayleigh_mp',
          seed=1, snrs=SNRS):
    return dict(bw=bw, mod=mod, prof=prof, nrx=nrx, coded=coded, n_sym=n_sym, cp=cp, paths=paths, chan=chan,
                seed=seed, snrs=snrs)


_G4 = (1.0, 0.9, 0.8, 0.7)
CODED_SNRS = (0.0, 4.0, 8.0, 14.0, 22.0)
SFBC_CASES = {
    'sfbc_pa20_u': _sfbc(20.0, '64-QAM'),
    'sfbc_pa20_c': _sfbc(20.0, '64-QAM', coded=True, snrs=(4.0, 9.0, 14.0, 20.0, 28.0)),
    'sfbc_pb20_u': _sfbc(20.0, '64-QAM', 'Pedestrian_B'),
    # (of seeds 1 .. 549 the first with a frame that decodes: the receiver's linear interpolation between
    # one TX's pilots, 12 subcarriers apart, does not follow 114 samples of delay spread, and only a
    # frame whose late taps are faded decodes)
    'sfbc_pb20_c': _sfbc(20.0, '64-QAM', 'Pedestrian_B', coded=True, snrs=(4.0, 9.0, 14.0, 20.0, 28.0), seed=549),
    'sfbc_vb20x_u': _sfbc(20.0, '16-QAM', 'Vehicular_B', cp='extended'),
    'sfbc_taps32_u': _sfbc(20.0, '16-QAM', None, paths=((0, 1, 31, 32), _G4)),
    'sfbc_taps33_u': _sfbc(20.0, '16-QAM', None, paths=((0, 33), (1.0, 0.8))),
    'sfbc_taps8_u': _sfbc(20.0, '16-QAM', None, paths=((0, 2, 5, 9, 14, 20, 27, 32), _G9[:8])),
    'sfbc_taps9_u': _sfbc(20.0, '16-QAM', None, paths=((0, 2, 5, 9, 14, 20, 27, 30, 32), _G9)),
    # (weak echoes: strong ones at these delays leave the reference's receiver an error floor)
    'sfbc_taps_cp_u': _sfbc(10.0, '16-QAM', None, paths=((0, 30, 72), (1.0, 0.2, 0.1))),
    'sfbc_taps_cp1_u': _sfbc(10.0, '16-QAM', None, paths=((0, 73), (1.0, 0.1))),
    'sfbc_vb5_u': _sfbc(5.0, 'QPSK', 'Vehicular_B', seed=403),      # the first seed with a frame under 1e-2
    'sfbc_vb5_c': _sfbc(5.0, 'QPSK', 'Vehicular_B', coded=True, snrs=(-4.0, 0.0, 4.0, 10.0, 18.0)),
    'sfbc_pa125_rx1_u': _sfbc(1.25, 'QPSK', nrx=1),
    'sfbc_pa15_c': _sfbc(15.0, '64-QAM', coded=True, snrs=(4.0, 9.0, 14.0, 20.0, 28.0)),
    'sfbc_rx3_u': _sfbc(20.0, '16-QAM', nrx=3), 'sfbc_rx4_u': _sfbc(20.0, '16-QAM', nrx=4),
    'sfbc_rx5_u': _sfbc(20.0, '16-QAM', nrx=5), 'sfbc_rx8_u': _sfbc(20.0, '16-QAM', nrx=8),
    'sfbc_sym15_u': _sfbc(20.0, '16-QAM', n_sym=15),
    'sfbc_awgn5_u': _sfbc(5.0, '16-QAM', chan='awgn'),
}
TXCH_MAXP, SFX_TL = 8, 32      # lte_mimo.hip


def sfbc_taps(cs, num):
    if cs['chan'] != 'rayleigh_mp':
        return np.zeros(0, dtype=int), np.zeros(0)
    if cs['paths'] is None:
        return O.itu_paths(num, cs['prof'])
    return np.array(cs['paths'][0]), np.array(cs['paths'][1], dtype=np.float64)


def sfbc_predicates(cs):
    """The dispatch predicates of select_mimo (lte_capi.hip) for a Philox run of
    the case without captures, restated from the case alone."""
    num = numerology(cs)
    dl, _ = sfbc_taps(cs, num)
    ray = cs['chan'] == 'rayleigh_mp'
    maxd, n_paths = (int(dl.max()), len(dl)) if ray else (0, 0)
    res = num.Nd & ~1
    n_sym = sfbc_geometry(cs, num)[0]
    txch = ray and num.N == 2048 and cs['nrx'] in (1, 2) and n_paths <= TXCH_MAXP and maxd <= SFX_TL and \
        maxd <= num.cp and res <= 8 * (num.N >> 3)
    rx_fuse = num.N == 2048 and cs['nrx'] <= 4 and res % 2 == 0 and (not cs['coded'] or num.bps in (4, 6))
    lp_fuse = ray and not txch and num.N >= 512 and maxd <= num.cp and n_paths <= TXCH_MAXP
    flat_fuse = not ray and num.N >= 512
    return dict(txch=txch, rx_fuse=rx_fuse, merge=txch and rx_fuse, lp_fuse=lp_fuse, flat_fuse=flat_fuse,
                maxd=maxd, n_paths=n_paths, n_est=(n_sym + 13) // 14)


def sfbc_geometry(cs, num):
    """(n_sym, n_bits, L) of the case's frame."""
    res = num.Nd & ~1
    if cs['coded']:
        _, seg = O.segment(O.attach_crc24a(np.zeros(TB, dtype=np.int64)))
        ncs = -(-sum(3 * p[0] + 12 for p in seg) // num.bps)
        n_sym, n_bits = -(-ncs // res), TB
    else:
        n_sym, n_bits = cs['n_sym'], uncoded_bits(num, cs['n_sym'], res)
    return n_sym, n_bits, n_sym * (num.N + num.cp)


def sfbc_frames(name, merged, seed=None, snrs=None):
    """The case's frames through mimo_oracle.simulate_sfbc(_coded) on
    philox.sfbc_draws; merged: the link noise folded into the RX noise draw (the
    device's default where the fused TX and the fused receiver both run)."""
    cs = SFBC_CASES[name]
    num = numerology(cs)
    seed = cs['seed'] if seed is None else seed
    n_sym, n_bits, L = sfbc_geometry(cs, num)
    dl, g = sfbc_taps(cs, num)
    paths = None if cs['paths'] is None else (dl, g)
    d_idx = MO.sfbc_data_idx(num)
    out = []
    for b, fid in enumerate(IDS):
        bits = P.payload_bits(seed, int(fid), n_bits).astype(np.int64)
        d = P.sfbc_draws(seed, int(fid), L, cs['nrx'], len(dl), merged=merged)
        snr = float((cs['snrs'] if snrs is None else snrs)[b])
        if cs['coded']:
            o = MO.simulate_sfbc_coded(num, bits, snr, cs['nrx'], cs['chan'], cs['prof'], draws=d, iters=ITERS,
                                       paths=paths)
            syms = o['symbols_rx_grid']
        else:
            o = MO.simulate_sfbc(num, bits, snr, cs['nrx'], cs['chan'], cs['prof'], draws=d, paths=paths)
            syms = o['symbols_rx']
        ys = o['signals_rx']
        # the receiver's inputs, for the captures: per RX the grids and the slot estimates
        Y = np.stack([np.stack(MO._fft_symbols(num, ys[r], n_sym)) for r in range(cs['nrx'])])     # [rx][sym][N]
        H = np.stack([np.stack([MO.mimo_estimate(num, Y[r, st], 2)[0] for st in range(0, n_sym, 14)])
                      for r in range(cs['nrx'])])                                                   # [rx][est][2][N]
        fr = dict(bits=bits, bits_rx=np.asarray(o['bits_received_array']).astype(np.uint8),
                  errs=int(o['bit_errors']), syms=syms, rx=np.stack(ys), H=H[:, :, :, d_idx], Yd=Y[:, :, d_idx],
                  n_bits=n_bits, n_sym=n_sym, L=L, snr=snr, npow=o['noise_power'])
        if cs['coded']:
            fr['crc'] = bool(o['crc_pass'])
        else:
            fr['margin'] = float(boundary_distances(syms, cs['mod']).min())
        out.append(fr)
    return out


def sfbc_sym_scale(fr):
    """Per RE, the size a relative error eps in the receiver's inputs takes in
    the combined symbol mean_r (conj(h) y + h conj(y')) / norm_r: mean over RX of
    2 max|Y_r| max|h| / norm_r of the RE's pair (the MRC form of
    tests/test_gpu_profiles.py, per Alamouti pair)."""
    H, Y = fr['H'], fr['Yd']                      # [rx][est][2][res], [rx][sym][res]
    nrx, n_sym, res = Y.shape
    sc = np.zeros((n_sym, res))
    for r in range(nrx):
        for l in range(n_sym):
            h0, h1 = H[r, l // 14, 0], H[r, l // 14, 1]
            a0, a1 = (h0[0::2] + h0[1::2]) / 2, (h1[0::2] + h1[1::2]) / 2
            nrm = np.abs(a0) ** 2 + np.abs(a1) ** 2 + 1e-10
            hm = np.max(np.abs(np.stack([h0[0::2], h0[1::2], h1[0::2], h1[1::2]])), axis=0)
            sc[l] += np.repeat(2 * np.max(np.abs(Y[r])) * hm / nrm, 2)
    return (sc / nrx).reshape(-1)


# ---------------------------------------------------------------------------
# Uncoded TM4 spatial multiplexing
def _sm(bw, mod, chan, prof='Pedestrian_A', ntx=4, nrx=4, rank=4, pmi=0, det='MMSE', vel=0.0, cp='normal', seed=1,
        snrs=(6.0, 14.0, 22.0, 30.0, 40.0), n_sym=3):
    return dict(bw=bw, mod=mod, chan=chan, prof=prof, ntx=ntx, nrx=nrx, rank=rank, pmi=pmi, det=det, vel=vel, cp=cp,
                seed=seed, snrs=snrs, n_sym=n_sym)


SM_CASES = {
    'sm_pb20_v3': _sm(20.0, '64-QAM', 'rayleigh_mp', 'Pedestrian_B', vel=3.0),
    'sm_va20_v30': _sm(20.0, '16-QAM', 'rayleigh_mp', 'Vehicular_A', vel=30.0),
    'sm_vb20x_v3': _sm(20.0, '16-QAM', 'rayleigh_mp', 'Vehicular_B', vel=3.0, cp='extended'),
    'sm_pb5_static': _sm(5.0, '16-QAM', 'rayleigh_mp', 'Pedestrian_B'),
    'sm_r2_pmi5_sic': _sm(5.0, '16-QAM', 'awgn', rank=2, pmi=5, det='SIC', snrs=(0.0, 8.0, 16.0, 24.0, 32.0)),
    'sm_r3_zf': _sm(10.0, '16-QAM', 'rayleigh_mp', nrx=3, rank=3, det='ZF', vel=3.0),
    'sm_22_pmi1_zf': _sm(1.25, 'QPSK', 'awgn', ntx=2, nrx=2, rank=2, pmi=1, det='ZF',
                         snrs=(0.0, 8.0, 16.0, 24.0, 32.0)),
    'sm_42_r1_mrc': _sm(5.0, '16-QAM', 'awgn', nrx=2, rank=1, pmi=3, det='MRC', snrs=(-4.0, 2.0, 8.0, 16.0, 26.0)),
    'sm_15': _sm(15.0, '64-QAM', 'awgn'),
}


def sm_n_paths(cs, num):
    return len(O.itu_paths(num, cs['prof'], spatial=True)[0]) if cs['chan'] == 'rayleigh_mp' else 0


def sm_frames(name, seed=None, snrs=None):
    """The case's frames through tm4_oracle.simulate_tm4(draws=philox.sm_draws).
    Per frame also, per data RE: kappa and mu_min of its subcarrier
    (spatial_coded_model.soft_rule), ||s|| of the subcarrier's detector output,
    the margin of every slicer input (SIC: of every stage's) and the
    disagreement of the Cholesky-order evaluation in units of eps kappa / mu_min
    ||s|| (r)."""
    cs = SM_CASES[name]
    num = numerology(cs)
    seed = cs['seed'] if seed is None else seed
    Nd, rank, det = num.Nd, cs['rank'], cs['det']
    n_sym = cs['n_sym']
    n_bits = uncoded_bits(num, n_sym)
    L = n_sym * (num.N + num.cp)
    n_dsc = -(-Nd // rank)
    P_ = sm_n_paths(cs, num)
    rule = 'MMSE' if det == 'SIC' else det
    out = []
    for b, fid in enumerate(IDS):
        bits = P.payload_bits(seed, int(fid), n_bits).astype(np.int64)
        d = P.sm_draws(seed, int(fid), L, cs['ntx'], cs['nrx'], cs['chan'], P_)
        snr = float((cs['snrs'] if snrs is None else snrs)[b])
        o = T.simulate_tm4(num, bits, snr, cs['ntx'], cs['nrx'], rank, det, cs['chan'], cs['prof'], cs['vel'], 2.0,
                           draws=d, pmi=cs['pmi'])
        s2 = 10 ** (-snr / 10)
        He, y = o['H_eff'], o['y']
        _, _, kap, mu = SCM.soft_rule(He, y, s2, rule)
        s_chol = SCM.soft_rule_chol(He, y, s2, rule, raw=True)            # [n_sym * n_dsc][rank]
        unit = EPS * kap / mu
        if det == 'SIC':     # the first stage's slicer input: the MMSE estimate of the strongest layer
            nrm = np.linalg.norm(s_chol, axis=1)
            dis = np.abs(s_chol[np.arange(len(y)), o['sic_order'][:, 0]] - o['sic_stages'][:, 0]) / (unit * nrm)
        else:
            nrm = np.linalg.norm(o['layers_rx'], axis=1)
            dis = np.abs(s_chol - o['layers_rx']) / (unit * nrm)[:, None]

        def per_re(v):                                   # [n_sym * n_dsc] -> per data RE
            return np.repeat(v, rank).reshape(n_sym, n_dsc * rank)[:, :Nd].reshape(-1)

        if det == 'SIC':     # every stage's slicer input, per subcarrier, against the subcarrier's margin
            # (a padding layer of the last subcarrier included: its decision is cancelled too)
            dist = boundary_distances(o['sic_stages'], cs['mod'])
            need = np.repeat(unit, rank)
        else:
            dist = boundary_distances(o['symbols_rx'], cs['mod'])
            need = per_re(unit)
        out.append(dict(bits=bits, bits_rx=np.asarray(o['bits_received_array']).astype(np.uint8),
                        errs=int(o['bit_errors']), syms=o['symbols_rx'], rx=np.stack(o['signals_rx']),
                        kappa=per_re(kap), mu=per_re(mu), s_norm=per_re(nrm), dist=dist, unit=need,
                        r=float(dis.max()), n_bits=n_bits, L=L, snr=snr, W=o['precoder_matrix'],
                        H=o['H_est'], npow=o['noise_power']))
    return out


def sm_margin_ok(frames, r):
    """Every slicer input at least max(1e-9, r eps kappa / mu) of the spacing from
    every decision boundary -> (ok, the smallest dist / need)."""
    worst = np.inf
    for fr in frames:
        need = np.maximum(BOUNDARY_MARGIN, r * fr['unit'])
        worst = min(worst, float(np.min(fr['dist'] / need)))
    return worst >= 1.0, worst


NOISE_FREE = (300.0,) * B


def frame_mix_ok(frames, floor):
    """An uncoded case's SNRs reach from frames with errors to a nearly clean
    one.  Nearly clean: a BER under NEARLY_CLEAN, or, on a channel the
    reference's estimator cannot follow (linear interpolation between one TX's
    pilots, 12 or 24 subcarriers apart, across a delay spread of 35 to 139
    samples: the BER stays at 0.05 to 0.45 whatever the SNR), a BER within
    NEARLY_CLEAN of the same frame's without noise.  floor(): the case's frames
    at NOISE_FREE, evaluated only then.  -> (ok, BERs, noise-free BERs or None)"""
    ber = [fr['errs'] / fr['n_bits'] for fr in frames]
    if max(ber) == 0:
        return False, ber, None
    if min(ber) < NEARLY_CLEAN:
        return True, ber, None
    fl = [fr['errs'] / fr['n_bits'] for fr in floor()]
    return min(a - b for a, b in zip(ber, fl)) < NEARLY_CLEAN, ber, fl
