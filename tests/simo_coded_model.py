"""The coded SIMO chain (LTE_CHAIN_SIMO_CODED, include/lte_phy.h) modelled from
the oracle's primitives (a helper of tests/test_simo_coded_host.py and
tests/test_gpu_simo_coded.py, not a conftest).

The definition: simulate_siso_coded's coding chain around simulate_simo's link
and combiner.  Everything here is oracle.coded_tx / channel_transmit (once per
RX) / demod_stream / estimate_periodic / the reference's scalar MRC sums as
oracle.simulate_simo restates them / llrs / coded_rx_decode, plus the one rule
that is this chain's own: sigma^2_eff = max(sigma^2 / clip(D, 1e-6, 1e6),
sigma^2 / 4), D = sum_r |H_r|^2, on either channel type."""
import numpy as np

FRAMES = 64 + 3          # one full 64-frame decoder group and a partial one
ITERS = 2
MIN_PASS = MIN_FAIL = 8

# The ladder: numerology, channel, TB size, RX count and the SNR window (dB)
# whose linspace over the 67 frames straddles the turbo cliff at 2 iterations.
CASES = {
    'A2': dict(bw=1.25, mod='QPSK', chan='awgn', prof='Pedestrian_A', n_bits=435, nrx=2, snr=(-2.0, 4.0)),
    'A4': dict(bw=1.25, mod='QPSK', chan='awgn', prof='Pedestrian_A', n_bits=435, nrx=4, snr=(-5.0, 1.0)),
    # K = 4096, 4096, 4160; 38 OFDM symbols = 3 estimation groups
    'B2': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=12217, nrx=2, snr=(3.0, 12.0)),
    # one RX and five: always k_rx_chest + k_rx_data (the fused receivers take 2..4 RX)
    'B1': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=2041, nrx=1, snr=(6.0, 20.0)),
    'B5': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=2041, nrx=5, snr=(1.0, 10.0)),
    'B3': dict(bw=5.0, mod='16-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=2041, nrx=3, snr=(2.0, 10.0)),
    'C2': dict(bw=20.0, mod='64-QAM', chan='rayleigh_mp', prof='Pedestrian_A', n_bits=6121, nrx=2, snr=(6.0, 18.0)),
    # N = 1024: the paired receiver.  With these draws the cliff sits near 6.9 dB (0..8 dB passes
    # 6 frames only), so the window reaches 10 dB: 23 pass, 44 fail
    'D4': dict(bw=10.0, mod='16-QAM', chan='rayleigh_mp', prof='Vehicular_A', n_bits=2041, nrx=4, snr=(1.0, 10.0)),
}


def numerology(O, cs):
    return O.Numerology(bandwidth=cs['bw'], modulation=cs['mod'])


def taps(O, num, cs):
    """(integer delays, linear gains) of the case's channel; none on AWGN."""
    if cs['chan'] != 'rayleigh_mp':
        return np.zeros(0, dtype=int), np.zeros(0)
    return O.itu_paths(num, cs['prof'])


def deinterleave_index(n_coded_syms, Nd):
    """src with coded symbol q = RE src[q] of the grid (the T/F interleaver of
    the coded chain: rows of Nd written, columns read)."""
    rows = -(-n_coded_syms // Nd)
    q = np.arange(n_coded_syms)
    return (q % Nd) * rows + q // Nd


def case_inputs(O, name, frames=FRAMES):
    """bits [F][n_bits], phases [F][nrx][P][16], unit normals [F][nrx][2][L] and
    SNRs [F]: frame f from RandomState(n_bits + f) -- bits, then phases, then
    normals -- in OFDMChannel.draw's layout."""
    cs = CASES[name]
    num = numerology(O, cs)
    dl, _ = taps(O, num, cs)
    L = len(O.coded_tx(num, np.zeros(cs['n_bits'], dtype=np.int64))['signal'])
    bits = np.zeros((frames, cs['n_bits']), dtype=np.uint8)
    ph = np.zeros((frames, cs['nrx'], len(dl), 16))
    z = np.zeros((frames, cs['nrx'], 2, L))
    for f in range(frames):
        rs = np.random.RandomState(cs['n_bits'] + f)
        bits[f] = rs.randint(0, 2, cs['n_bits'])
        ph[f] = 2 * np.pi * rs.rand(cs['nrx'], len(dl), 16)
        z[f] = rs.standard_normal((cs['nrx'], 2, L))
    return dict(bits=bits, ph=ph, z=z, snrs=np.linspace(cs['snr'][0], cs['snr'][1], frames), L=L)


def draws_of(ph, z):
    """One frame's injected numbers in the oracle's `draws` format, per RX."""
    return [{'phases': [ph[r, p] for p in range(ph.shape[1])], 'z_re': z[r, 0], 'z_im': z[r, 1]}
            for r in range(z.shape[0])]


def combine(O, num, rxs):
    """MRC of the received streams: (z [n_sym * Nd] in grid order, D [n_grp][Nd],
    sum_r max|Y_r|^2 over the data REs: the size of the combiner's inputs).
    num = sum_r conj(H_r) Y_r in RX order in the reference's scalar form
    (oracle.simulate_simo), D = sum_r |H_r|^2, z = num / (D + 1e-10); the
    estimate of each RX is its first symbol's of every 14-symbol group."""
    num_acc = den = Dg = None
    ymax2 = 0.0
    for y in rxs:
        Yf = O.demod_stream(num, y)
        Hs, _ = O.estimate_periodic(num, Yf)
        Y = Yf[:, num.data_idx].reshape(-1)
        H = np.stack(Hs)[:, num.data_idx].reshape(-1)
        Hg = np.stack(Hs[::14])[:, num.data_idx]                      # [n_grp][Nd]
        if num_acc is None:
            num_acc = np.zeros(len(Y), dtype=complex)
            Dg = np.zeros(Hg.shape)
        hr, hi, yr, yi = H.real, -H.imag, Y.real, Y.imag
        prod = np.empty(len(Y), dtype=complex)
        prod.real = hr * yr - hi * yi
        prod.imag = hr * yi + hi * yr
        num_acc += prod
        Dg += np.array([[np.abs(h) ** 2 for h in row] for row in Hg])
        ymax2 += float(np.max(np.abs(Y))) ** 2
    n_sym = len(num_acc) // num.Nd
    den = Dg[np.arange(n_sym) // 14].reshape(-1)
    return num_acc / (den + 1e-10), Dg, ymax2


def symbol_scale(Dg, ymax2, n_sym):
    """Per RE, the size an error of the inputs has in z: sqrt(sum_r max|Y_r|^2) /
    sqrt(D) (a relative error e of every Y_r and H_r moves z by a few e of it)."""
    return np.sqrt(ymax2) / np.sqrt(Dg[np.arange(n_sym) // 14].reshape(-1))


def sigma2_eff(D, snr_db):
    s2 = 1.0 / (10 ** (snr_db / 10))
    return np.maximum(s2 / np.clip(D, 1e-6, 1e6), s2 / 4.0)


def soft_output(O, num, zc, Dg, coded_len, snr_db):
    """(LLRs [coded_len] in coded order, z and D per coded symbol) of the
    combiner's output: T/F de-interleave, sigma^2_eff, max-log demapper."""
    ncs = coded_len // num.bps
    src = deinterleave_index(ncs, num.Nd)
    n_sym = len(zc) // num.Nd
    D = Dg[np.arange(n_sym) // 14].reshape(-1)[src]
    sd = zc[src]
    L = O.llrs(sd, sigma2_eff(D, snr_db), num.modulation)
    return L[:coded_len], sd, D


def frame(O, num, cs, bits, snr_db, draws, fD=0.0, iters=ITERS, f32=False):
    """One frame through the model.  draws: per RX {'phases', 'z_re', 'z_im'}."""
    bits = np.asarray(bits).astype(np.int64)
    tx = O.coded_tx(num, bits)
    rxs = [O.channel_transmit(num, tx['signal'], cs['chan'], snr_db, cs['prof'], fD, d) for d in draws]
    zc, Dg, ymax2 = combine(O, num, rxs)
    coded_len = len(tx['coded'])
    L, sd, D = soft_output(O, num, zc, Dg, coded_len, snr_db)
    dec, ok = O.coded_rx_decode(L.astype(np.float32) if f32 else L, tx['plan'], tx['rm_lens'], iters, f32_model=f32)
    return dict(tx=tx, rxs=rxs, z=zc, Dg=Dg, z_scale=symbol_scale(Dg, ymax2, len(zc) // num.Nd), llr=L,
                symbols_rx=sd, channel_gain=D, bits_rx=np.asarray(dec), crc=bool(ok),
                errs=int(np.sum(bits != dec)))


def noise_powers(O, num, cs, sig, snr_db, draws, fD=0.0):
    """Per RX: mean |y|^2 of the faded, noiseless stream / SNR (the link's rule)."""
    dl, g = taps(O, num, cs)
    out = []
    for d in draws:
        y = O.multipath(sig, dl, g, d['phases'], fD, num.fs) if cs['chan'] == 'rayleigh_mp' else sig
        out.append(np.mean(np.abs(y) ** 2) / 10 ** (snr_db / 10))
    return np.array(out)


def decode_llrs(O, num, seg, coded_len, llr_re, iters=ITERS, f32=False):
    """The oracle's RX decode of a captured LLR array (RE order, [n_re * bps])."""
    src = deinterleave_index(coded_len // num.bps, num.Nd)
    L = np.asarray(llr_re, dtype=np.float64).reshape(-1, num.bps)[src].reshape(-1)[:coded_len]
    return O.coded_rx_decode(L, seg, [3 * p[0] + 12 for p in seg], iters, f32_model=f32)


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


def philox_frame(O, P, num, cs, seed, frame_id, snr_db, fD=0.0, iters=ITERS):
    """One run_grid frame: the frame's Philox payload and LTE_CHAIN_SIMO's
    streams (philox.siso_draws) through the model."""
    bits = P.payload_bits(seed, frame_id, cs['n_bits'])
    L = len(O.coded_tx(num, bits)['signal'])
    dl, _ = taps(O, num, cs)
    return frame(O, num, cs, bits, snr_db, P.siso_draws(seed, frame_id, L, len(dl), cs['nrx']), fD=fD, iters=iters)


_CACHE = {}


def case_frames(O, name):
    """The model's 67 frames of a ladder case on case_inputs (computed once)."""
    if name not in _CACHE:
        cs = CASES[name]
        num = numerology(O, cs)
        inp = case_inputs(O, name)
        _CACHE[name] = (inp, [frame(O, num, cs, inp['bits'][f], float(inp['snrs'][f]),
                                    draws_of(inp['ph'][f], inp['z'][f])) for f in range(FRAMES)])
    return _CACHE[name]
