"""HARQ re-packing of the unacknowledged frames, modelled on tests/harq_model.py
(a helper of tests/test_harq_repack_host.py and tests/test_gpu_harq_repack.py,
not a conftest).

The rule (include/lte_phy.h, lte_plan_set_harq_repack): group g of the B frames
has valid = min(64, B - 64 g) lanes and `active` of them not acknowledged; it
is finished (active = 0), full (active = valid) or mixed.  M = mixed groups, A =
their active frames, P = ceil(A / 64); a round t >= 1 on the skip-aware
decoders packs iff M >= 1, P < M and P <= cap.  In a round that packs, the
acknowledged frames of mixed groups are not decoded again: their decisions stay
those of the round that acknowledged them."""
import numpy as np

import harq_model as M


def pack_cap(groups):
    """Packed groups a plan of `groups` 64-frame groups holds (turbo_pack_cap)."""
    return -(-groups // 4) if groups > 4 else 1


def classes(acked):
    """Per group 'finished' / 'full' / 'mixed' and its active frames."""
    acked = np.asarray(acked) != 0
    out = []
    for g in range(-(-len(acked) // 64)):
        lanes = acked[g * 64:(g + 1) * 64]
        active = int(np.sum(~lanes))
        out.append(('finished' if active == 0 else 'full' if active == len(lanes) else 'mixed', active))
    return out


def rule(acked, cap):
    """The rule restated: M, A, P, pack and the decoder groups per slot without
    (full + mixed) and with re-packing (full + P when it packs)."""
    cl = classes(acked)
    mixed = [a for c, a in cl if c == 'mixed']
    m, a = len(mixed), sum(mixed)
    p = -(-a // 64)
    pack = m >= 1 and p < m and p <= cap
    off = sum(1 for c, _ in cl if c != 'finished')
    return {'M': m, 'A': a, 'P': p, 'pack': pack, 'waves_off': off, 'waves_on': off - m + p if pack else off}


class Process(M.Process):
    """harq_model.Process with the setting on: cap packed groups.  round()
    also returns 'repack': the round's rule (None in round 0) and its state."""

    def __init__(self, *a, cap, **kw):
        super().__init__(*a, **kw)
        self.cap = cap

    def round(self, t, llr):
        O, rv = self.O, self.rv_seq[t]
        fin = self.finished_groups() if t >= 1 else []
        info = rule(self.ack, self.cap) if t >= 1 else None
        pack = bool(info and info['pack'] and self.skip)
        before = self.ack.copy()
        dec = O.turbo_decode_f32_model if self.f32 else O.turbo_decode
        for b in range(self.B):
            off = 0
            for r, (p, E) in enumerate(zip(self.plan, self.Es)):
                dm = O.rate_dematch(np.asarray(llr[b][off:off + E], dtype=np.float64), p[0], rv).astype(self.dt)
                self.soft[b][r] = self.soft[b][r] + dm
                off += E
            if self.skip and b // 64 in fin:
                continue
            if pack and before[b]:
                continue                                      # acknowledged, in a packed mixed group: not decoded again
            tbc = O.desegment([dec(s, p[0], self.iters) for s, p in zip(self.soft[b], self.plan)], self.plan)
            ok = bool(O.check_crc24a(tbc))
            self.bits_rx[b] = tbc[:-24]
            if not self.ack[b]:
                self.tx_used[b] = t + 1
                self.err[b] = int(np.sum(self.bits_rx[b] != self.tx[b]))
                self.ok[b] = ok
                self.ack[b] = ok
        state = 'none' if t == 0 else 'packed' if pack else 'in_place'
        return dict(bits_rx=self.bits_rx.copy(), crc_ok=self.ok.copy(), frame_errors=self.err.copy(),
                    tx_used=self.tx_used.copy(), skipped=len(fin) if self.skip else 0, repack=info, state=state,
                    acked_before=before)
