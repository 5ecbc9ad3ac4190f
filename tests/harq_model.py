"""HARQ with soft combining, modelled from the oracle's primitives (a helper of
tests/test_harq_host.py and tests/test_gpu_harq.py, not a conftest).

The definition (include/lte_phy.h, lte_plan_create_harq): transmission t of a
transport block is rate matched with rv_seq[t] to E_r bits per code block
(split(): 36.212 5.1.4.1.2 with one layer; G = 0 keeps 3K + 12), the receiver
adds rate_dematch(llr_t, K, rv_t) to the sum of the rounds before, decodes the
sum, and a frame is acknowledged in the first round whose CRC-24A passes.
Everything here is oracle.attach_crc24a / segment / turbo_encode / rate_match /
bits_to_symbols / rate_dematch / turbo_decode(_f32_model) / desegment /
check_crc24a plus the bookkeeping."""
import numpy as np

GOLDEN64 = 0x9E3779B97F4A7C15


def seed_t(seed, t):
    """Key of round t's channel and noise streams (the payload keeps `seed`)."""
    return (int(seed) + int(t) * GOLDEN64) % (1 << 64)


def split(O, n_bits, bps, G):
    """(K_r, E_r) of a TB of n_bits (+ 24 CRC) sent in G coded bits; ValueError
    where the plan refuses G."""
    Ks = [p[0] for p in O.segmentation_plan(n_bits + 24)]
    C = len(Ks)
    if G == 0:
        return Ks, [3 * K + 12 for K in Ks]
    if G < 0 or G % bps:
        raise ValueError('G must be a non-negative multiple of bps')
    Gp = G // bps
    gamma = Gp % C
    Es = [bps * (Gp // C if r <= C - gamma - 1 else -(-Gp // C)) for r in range(C)]
    for K, E in zip(Ks, Es):
        if not bps <= E <= 3 * K + 18:
            raise ValueError(f'E = {E} outside [bps, 3K + 18] for K = {K}')
    return Ks, Es


def encode(O, bits):
    """(turbo-encoded code blocks, segmentation plan) of one payload."""
    cbs, plan = O.segment(O.attach_crc24a(np.asarray(bits)))
    return [O.turbo_encode(cb) for cb in cbs], plan


def tx_qam(O, num, enc, plan, Es, rv):
    """QAM symbols of one transmission and the grid RE each lands on (the T/F
    interleaver of the coded chain: rows of Nd written, columns read)."""
    coded = np.concatenate([O.rate_match(e, E, p[0], rv) for e, p, E in zip(enc, plan, Es)])
    qam = O.bits_to_symbols(coded, num.modulation)
    q = np.arange(len(qam))
    rows = -(-len(qam) // num.Nd)
    return qam, (q % num.Nd) * rows + q // num.Nd


def tx_signal(O, num, qam):
    """The time-domain frame of one transmission: T/F interleaver, grid mapping
    and OFDM modulation as oracle.coded_tx does them for its own symbols."""
    perm, rows, total = O.tf_interleave_perm(len(qam), num.Nd)
    inter = np.pad(qam, (0, total - len(qam)))[perm]
    return O.ofdm_symbols_tx(num, inter.reshape(rows, num.Nd), O.pilots(0, num.Np))


def llr_coded_order(llr_re, num, coded_len):
    """A captured LLR array (RE order, [n_re * bps]) in coded-bit order."""
    ncs = coded_len // num.bps
    rows = -(-ncs // num.Nd)
    q = np.arange(ncs)
    src = (q % num.Nd) * rows + q // num.Nd
    return np.asarray(llr_re).reshape(-1, num.bps)[src].reshape(-1)[:coded_len]


class Process:
    """The receiver side of one HARQ process of B frames.  round(t, llr) takes
    the round's LLRs [B][coded_len] in coded order and returns what the plan
    reports after it: bits_rx (the last decode performed per frame), crc_ok,
    frame_errors, tx_used (all latched) and the number of 64-frame groups that
    were finished before the round (those the decoder skips when skip=True)."""

    def __init__(self, O, plan, Es, rv_seq, tx_bits, iters, f32=False, skip=True):
        self.O, self.plan, self.Es, self.rv_seq = O, plan, list(Es), list(rv_seq)
        self.tx = np.asarray(tx_bits)
        self.B = len(self.tx)
        self.iters, self.f32, self.skip = iters, f32, skip
        self.dt = np.float32 if f32 else np.float64
        self.soft = [[np.zeros(3 * p[0] + 12, dtype=self.dt) for p in plan] for _ in range(self.B)]
        self.bits_rx = np.zeros_like(self.tx)
        self.ack = np.zeros(self.B, dtype=bool)
        self.tx_used = np.zeros(self.B, dtype=np.uint8)
        self.err = np.zeros(self.B, dtype=np.uint32)
        self.ok = np.zeros(self.B, dtype=np.uint8)

    def finished_groups(self):
        return [g for g in range(-(-self.B // 64)) if self.ack[g * 64:(g + 1) * 64].all()]

    def round(self, t, llr):
        O, rv = self.O, self.rv_seq[t]
        fin = self.finished_groups() if t >= 1 else []
        dec = O.turbo_decode_f32_model if self.f32 else O.turbo_decode
        for b in range(self.B):
            off = 0
            for r, (p, E) in enumerate(zip(self.plan, self.Es)):
                dm = O.rate_dematch(np.asarray(llr[b][off:off + E], dtype=np.float64), p[0], rv).astype(self.dt)
                self.soft[b][r] = self.soft[b][r] + dm        # round order, the plan's arithmetic
                off += E
            if self.skip and b // 64 in fin:
                continue                                      # not decoded again: decisions stay
            tbc = O.desegment([dec(s, p[0], self.iters) for s, p in zip(self.soft[b], self.plan)], self.plan)
            ok = bool(O.check_crc24a(tbc))
            self.bits_rx[b] = tbc[:-24]
            if not self.ack[b]:
                self.tx_used[b] = t + 1
                self.err[b] = int(np.sum(self.bits_rx[b] != self.tx[b]))
                self.ok[b] = ok
                self.ack[b] = ok
        return dict(bits_rx=self.bits_rx.copy(), crc_ok=self.ok.copy(), frame_errors=self.err.copy(),
                    tx_used=self.tx_used.copy(), skipped=len(fin) if self.skip else 0)

    def counts(self, snr_index=None, n_snr=1):
        """The plan's counts after the last round: per SNR row {bit errors, bits,
        block errors, blocks} of the latched state."""
        si = np.zeros(self.B, dtype=int) if snr_index is None else np.asarray(snr_index)
        c = np.zeros((n_snr, 4), dtype=np.uint64)
        np.add.at(c[:, 0], si, self.err.astype(np.uint64))
        np.add.at(c[:, 1], si, np.uint64(self.tx.shape[1]))
        np.add.at(c[:, 2], si, (self.ok == 0).astype(np.uint64))
        np.add.at(c[:, 3], si, np.uint64(1))
        return c


def histogram(tx_used, crc_ok, max_tx):
    """[never, acknowledged after 1, .., after max_tx]."""
    return np.bincount(np.where(np.asarray(crc_ok) != 0, tx_used, 0), minlength=max_tx + 1).tolist()
