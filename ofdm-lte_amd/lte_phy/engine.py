"""Plan cache and batch runner over the C ABI (lte_plan_create / lte_run).

A plan is one device workspace for one configuration (numerology, chain,
channel, payload size, capacity).  `Plan.run` executes the whole
TX -> channel -> RX (-> turbo) chain for a batch of frames on the GPU and
returns counters and any requested host captures.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import numpy as np

from . import _capi as C


def chain_is_coded(chain):
    """Plan.coded: the chain runs the coding chain (encoder, dematch, turbo, CRC)."""
    return bool(C.chain_info(chain).coded)


def chain_is_mimo(chain):
    """Plan.mimo: a multi-antenna chain (run_mimo, the multi-antenna capture shapes)."""
    return C.chain_info(chain).family == C.FAMILY_MIMO


class RunResult(dict):
    """Plan.run's outputs by name (counts, frame_errors, the captures); .path:
    the kernel path the run took (lte_run_path) as a dict of its fields."""
    path = None


REPACK_DEFAULT = 1   # the boundary repack=True stands for
REPACK_STATES = ('none', 'packed', 'in_place')   # lte_plan_repack_info's 0 / 1 / 2
# lte_plan_pipe_info's reason codes 0 .. 8
PIPE_REASONS = ('pipelined', 'off', 'chain', 'path', 'stages', 'capture', 'inject', 'decoder', 'one_slice')


def repack_boundary(repack, early_stop, turbo_iters):
    """The re-packing boundary `after` a repack= keyword stands for (0: off;
    True: REPACK_DEFAULT), checked against early_stop and turbo_iters.  Raises
    ValueError; touches no device."""
    if repack is None or repack is False:
        return 0
    after = REPACK_DEFAULT if repack is True else int(repack)
    if after == 0:
        return 0
    if not early_stop:
        raise ValueError('repack re-packs the blocks early stop leaves undecided: it needs early_stop=True')
    if not 1 <= after < int(turbo_iters):
        raise ValueError(f'repack: the boundary must satisfy 1 <= after < turbo_iters (after = {after}, '
                         f'turbo_iters = {int(turbo_iters)})')
    return after


def turbo_scale_value(scale):
    """The extrinsic scale a turbo_scale= keyword stands for (None: 1.0, off),
    checked to lie in (0, 1].  Raises ValueError; touches no device."""
    if scale is None:
        return 1.0
    s = float(scale)
    if not 0.0 < s <= 1.0:   # (NaN fails both comparisons)
        raise ValueError(f'turbo_scale must satisfy 0 < scale <= 1 (got {scale!r})')
    return s


class Plan:
    def __init__(self, *, N, Nc, cp_len, bps, n_sym, chain, channel, num_rx=1, delays=(), gains=(), fD=0.0,
                 fs=0.0, n_bits, turbo_iters=8, max_frames=1, cell_id=0, num_tx=1, rank=0, detector=0,
                 precoder=(), sc_fdm=0, bf_adaptive=0, no_equalization=0, precision=None, early_stop=False,
                 harq=None, harq_repack=False, repack=None, turbo_scale=None):
        if harq_repack and harq is None:   # before any device call
            raise ValueError('harq_repack re-packs the unacknowledged frames of a HARQ process: it needs harq=')
        after = repack_boundary(repack, early_stop, turbo_iters)   # before any device call
        scale = turbo_scale_value(turbo_scale)                     # likewise
        C.device_init()
        d = C.PlanDesc()
        d.N, d.Nc, d.cp_len, d.bps, d.n_sym = N, Nc, cp_len, bps, n_sym
        d.chain, d.channel, d.num_rx = chain, channel, num_rx
        d.n_paths = len(delays)
        if d.n_paths > C.MAX_PATHS:
            raise ValueError('too many multipath taps')
        for i, (dl, g) in enumerate(zip(delays, gains)):
            d.delays[i] = int(dl)
            d.gains[i] = float(g)
        d.fD, d.fs = float(fD), float(fs)
        d.n_bits, d.turbo_iters, d.max_frames, d.cell_id = int(n_bits), int(turbo_iters), int(max_frames), cell_id
        d.num_tx = int(num_tx)
        d.rank, d.detector, d.sc_fdm, d.bf_adaptive = int(rank), int(detector), int(sc_fdm), int(bf_adaptive)
        d.no_equalization = int(no_equalization)
        # float64 (the reference's arithmetic) unless 'f32' is asked for
        d.precision = C.PREC_F64 if C.precision_of(precision) == 'f64' else C.PREC_F32
        if rank and num_tx <= 4 and rank <= 4:   # W [num_tx][rank] -> the [4][4] table of lte_plan_desc.precoder
            #                                    (larger arrays: lte_plan_create rejects them, LTE_EUNSUP)
            W = np.asarray(precoder, dtype=np.complex128).reshape(int(num_tx), int(rank))
            for t in range(W.shape[0]):
                for c in range(W.shape[1]):
                    d.precoder[(t * 4 + c) * 2] = float(W[t, c].real)
                    d.precoder[(t * 4 + c) * 2 + 1] = float(W[t, c].imag)
        self.desc = d
        h = ctypes.c_void_p()
        # HARQ (lte_plan_create_harq; coded SISO chain): dict(max_tx=4, rv_seq=(0, 2, 3, 1),
        # coded_bits=0), coded_bits = G, the coded bits per transmission (0: 3K + 12 per code block)
        self.harq = None
        if harq is not None:
            hq = dict(max_tx=4, rv_seq=(0, 2, 3, 1), coded_bits=0)
            unknown = set(harq) - set(hq)
            if unknown:
                raise ValueError(f'harq: unknown keys {sorted(unknown)}')
            hq.update(harq)
            hq['max_tx'], hq['coded_bits'] = int(hq['max_tx']), int(hq['coded_bits'] or 0)
            hq['rv_seq'] = tuple(int(v) for v in hq['rv_seq'])
            if not 1 <= hq['max_tx'] <= 8 or len(hq['rv_seq']) < hq['max_tx']:
                raise ValueError('harq: max_tx must be in 1..8 with one rv_seq entry per transmission')
            hd = C.HarqDesc()
            hd.max_tx, hd.G = hq['max_tx'], hq['coded_bits']
            for t in range(hq['max_tx']):
                hd.rv_seq[t] = hq['rv_seq'][t]
            self.harq = hq
            C.check(C.load().lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)))
        else:
            C.check(C.load().lte_plan_create(ctypes.byref(d), ctypes.byref(h)))
        self.h = h
        info = np.zeros(8, dtype=np.int64)
        C.check(C.load().lte_plan_info(h, C.ptr(info, C.c_i64)))
        self.L, self.n_sym, self.Nd, self.Np, self.n_grp, self.n_cb, self.coded_bits, self.n_re_bits = \
            (int(v) for v in info)
        self.precision = 'f64' if C.load().lte_plan_precision(h) == C.PREC_F64 else 'f32'
        # element types of in_signal and the real / complex captures
        self.cdt = np.complex128 if self.precision == 'f64' else np.complex64
        self.rdt = np.float64 if self.precision == 'f64' else np.float32
        self.num_rx, self.N, self.bps, self.n_bits, self.max_frames = num_rx, N, bps, int(n_bits), int(max_frames)
        self.chain = chain
        self.num_tx = int(num_tx)
        self.coded = chain_is_coded(chain)
        self.bf = C.chain_info(chain).family == C.FAMILY_BF
        self.mimo = chain_is_mimo(chain)
        sfbc = C.chain_info(chain).mode == C.MODE_SFBC
        # multi-antenna geometry (lte_capi.hip lte_plan_create): REs per OFDM symbol,
        # data SCs carrying data, channel estimates per frame
        self.res = (self.Nd & ~1) if sfbc else self.Nd
        self.rank = int(rank) if rank else self.num_tx
        self.n_dsc = self.res if sfbc else -(-self.Nd // max(1, self.rank))
        self.n_est = self.n_grp if sfbc else self.n_sym
        # per-TX CRS subsets pilots[t::step], step = min(num_tx, 4) (lte_capi.hip
        # plan_mimo_tables, core/mimo_channel_estimator_periodic.py:75-107): the
        # largest subset is what the spatial receiver hands the detector per
        # (RX, estimate, TX) on the pilot-estimate path (LTE_SPATIAL_HP)
        self.cp_len, self.channel = int(cp_len), int(channel)
        self.n_paths, self.max_delay = len(delays), int(max(delays)) if len(delays) else 0
        self.pilots_per_tx = -(-self.Np // min(max(1, self.num_tx), 4))
        # CRC early termination of the turbo decoder (lte_plan_set_early_stop; coded
        # chains only): run() then also returns 'turbo_iters_used' [B, n_cb]
        self.early_stop = bool(early_stop)
        if self.early_stop:
            C.check(C.load().lte_plan_set_early_stop(h, 1))
        # re-packing of the blocks still undecided after `repack` iterations
        # (lte_plan_set_early_stop_repack; 0: off): run() then also returns 'repack_info'
        self.repack = 0
        if after:
            self.set_repack(after)
        # extrinsic scaling of the decoders (lte_plan_set_turbo_scale; coded chains only; 1.0: off)
        if scale != 1.0:
            self.set_turbo_scale(scale)
        # re-packing of the unacknowledged frames of mixed decoder groups (lte_plan_set_harq_repack;
        # HARQ plans only): run() then also returns 'harq_repack_info'
        self.harq_repack = False
        if harq_repack:
            self.set_harq_repack(True)

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                C.load().lte_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------
    def run(self, snr_db, **kw):
        """One batch through lte_run (keywords: _args) -> RunResult."""
        a, out, keep = self._args(snr_db, **kw)
        path = self._path(a)   # before the run: a HARQ plan's round is consumed by it
        C.check(C.load().lte_run(self.h, ctypes.byref(a)))
        out.path = path
        if self.early_stop and (a.stages & C.STAGE_RX):
            used = np.zeros((a.n_frames, self.n_cb), dtype=np.uint8)
            C.check(C.load().lte_plan_turbo_iters_used(self.h, C.ptr(used, C.U8), used.size))
            out['turbo_iters_used'] = used
            if self.repack:
                out['repack_info'] = self.repack_info()
        if self.harq is not None and (a.stages & C.STAGE_RX):   # the process's state after this round
            used = np.zeros(a.n_frames, dtype=np.uint8)
            C.check(C.load().lte_plan_harq_tx_used(self.h, C.ptr(used, C.U8), used.size))
            out['tx_used'] = used
            out['harq_info'] = self.harq_info()
            if self.harq_repack:
                out['harq_repack_info'] = self.harq_repack_info()
        del keep
        return out

    # ------------------------------------------------------------------ re-packing
    def set_repack(self, repack):
        """Switch re-packing to the boundary `repack` (True: the default one), or
        off (0 / None / False); the packed arrays stay allocated."""
        after = repack_boundary(repack, self.early_stop, self.desc.turbo_iters)
        C.check(C.load().lte_plan_set_early_stop_repack(self.h, after))
        self.repack = after

    def repack_info(self):
        """lte_plan_repack_info as a dict: after, n_cb and per code block slot the
        blocks undecided at the boundary, the 64-block groups that ran the
        remaining iterations and the state ('none' / 'packed' / 'in_place')."""
        v = np.zeros(2 + 3 * self.n_cb, dtype=np.int64)
        C.check(C.load().lte_plan_repack_info(self.h, C.ptr(v, C.c_i64), len(v)))
        t = v[2:].reshape(self.n_cb, 3)
        return {'after': int(v[0]), 'n_cb': int(v[1]), 'undecided': [int(x) for x in t[:, 0]],
                'groups': [int(x) for x in t[:, 1]], 'state': [REPACK_STATES[int(x)] for x in t[:, 2]]}

    # ------------------------------------------------------------------ coded SISO pipeline
    def pipe_info(self):
        """lte_plan_pipe_info of the last run as a dict: slices (0: the run was
        serial), groups (64-frame groups per slice) and reason (why it was serial)."""
        v = np.zeros(3, dtype=np.int64)
        C.check(C.load().lte_plan_pipe_info(self.h, C.ptr(v, C.c_i64), len(v)))
        return {'slices': int(v[0]), 'groups': int(v[1]), 'reason': PIPE_REASONS[int(v[2])]}

    # ------------------------------------------------------------------ extrinsic scaling
    def set_turbo_scale(self, scale):
        """Scale the decoders' extrinsic by `scale`, 0 < scale <= 1 (scaled
        max-log-MAP; lte_plan_set_turbo_scale); None or 1 switches it off."""
        C.check(C.load().lte_plan_set_turbo_scale(self.h, turbo_scale_value(scale)))

    @property
    def turbo_scale(self):
        return float(C.load().lte_plan_turbo_scale(self.h))

    # ------------------------------------------------------------------ HARQ
    def harq_round(self, t):
        """The next run() is transmission t of the process (lte_plan_harq_set_round):
        0 starts a new one, t >= 1 must follow round t - 1 with the same frames."""
        C.check(C.load().lte_plan_harq_set_round(self.h, int(t)))

    def harq_info(self):
        """lte_plan_harq_info as a dict: max_tx, round / rv / skipped (decoder groups)
        of the last run, coded_bits (G as sent), E (per code block)."""
        v = np.zeros(6 + self.n_cb, dtype=np.int64)
        C.check(C.load().lte_plan_harq_info(self.h, C.ptr(v, C.c_i64), len(v)))
        return {'max_tx': int(v[0]), 'round': int(v[1]), 'rv': int(v[2]), 'skipped': int(v[3]),
                'coded_bits': int(v[4]), 'n_cb': int(v[5]), 'E': [int(e) for e in v[6:]]}

    def set_harq_repack(self, on):
        """Switch the re-packing of unacknowledged frames on or off
        (lte_plan_set_harq_repack); the packed arrays stay allocated."""
        if self.harq is None:
            raise ValueError('harq_repack needs a plan made with harq=')
        C.check(C.load().lte_plan_set_harq_repack(self.h, 1 if on else 0))
        self.harq_repack = bool(on)

    def harq_repack_info(self):
        """lte_plan_harq_repack_info of the last run as a dict: on, state ('none':
        round 0 / 'packed' / 'in_place'), M (mixed groups), A (their active
        frames), P (packed groups), cap and waves (decoder groups run per slot)."""
        v = np.zeros(7, dtype=np.int64)
        C.check(C.load().lte_plan_harq_repack_info(self.h, C.ptr(v, C.c_i64), len(v)))
        return {'on': bool(v[0]), 'state': REPACK_STATES[int(v[1])], 'M': int(v[2]), 'A': int(v[3]), 'P': int(v[4]),
                'cap': int(v[5]), 'waves': int(v[6])}

    def run_harq(self, snr_db, **kw):
        """One HARQ process: the rounds 0 .. max_tx - 1 with the same arguments,
        stopping after the first round that leaves no frame unacknowledged.
        Returns tx_used / crc_ok / frame_errors (latched), counts (after the
        last round run), counts_by_round [max_tx, n_snr, 4] (rounds not run
        repeat the last), rounds_run, skipped (decoder groups per round run),
        with capture= a list `rounds` of each round's captures, and with
        harq_repack on the per-round list harq_repack_info."""
        if self.harq is None:
            raise ValueError('run_harq needs a plan made with harq=')
        capture = tuple(kw.get('capture', ()))
        cbr, rounds, skipped, packs, r = [], [], [], [], None
        for t in range(self.harq['max_tx']):
            self.harq_round(t)
            r = self.run(snr_db, **kw)
            cbr.append(r['counts'].copy())
            skipped.append(r['harq_info']['skipped'])
            if self.harq_repack:
                packs.append(r['harq_repack_info'])
            if capture:
                rounds.append({k: r[k] for k in capture})
            if bool(np.all(r['crc_ok'] != 0)):
                break
        out = RunResult(counts=r['counts'], frame_errors=r['frame_errors'], crc_ok=r['crc_ok'],
                        tx_used=r['tx_used'], rounds_run=len(cbr), skipped=skipped,
                        counts_by_round=np.stack(cbr + [cbr[-1]] * (self.harq['max_tx'] - len(cbr))))
        out.path = r.path
        if capture:
            out['rounds'] = rounds
        if self.harq_repack:
            out['harq_repack_info'] = packs
        return out

    def path(self, snr_db, **kw):
        """The kernel path run(snr_db, **kw) would take under the current
        environment switches, without running anything."""
        a, _, keep = self._args(snr_db, **kw)
        p = self._path(a)
        del keep
        return p

    def _path(self, a):
        buf = ctypes.create_string_buffer(256)
        C.check(C.load().lte_run_path(self.h, ctypes.byref(a), buf, len(buf)))
        return dict(kv.split('=', 1) for kv in buf.value.decode().split())

    def _args(self, snr_db, *, snr_index=None, n_snr=1, seed=0, frame_ids=None, frame_id0=0, bits=None,
              bits_broadcast=False, phases=None, phases_broadcast=False, noise=None, noise_broadcast=False,
              stages=C.STAGE_ALL, in_signal=None, capture=(), link_noise=None, link_h=None, link_broadcast=False):
        snr = np.ascontiguousarray(np.atleast_1d(snr_db), dtype=np.float64)   # float64 as the reference (ABI 3)
        B = len(snr)
        a = C.RunArgs()
        a.n_frames = B
        a.snr_db = C.ptr(snr, C.F64)
        keep = [snr]
        if snr_index is not None:
            si = np.ascontiguousarray(snr_index, dtype=np.int32)
            keep.append(si)
            a.snr_index = C.ptr(si, C.I32)
        a.n_snr = int(n_snr)
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if frame_ids is not None:
            fi = np.ascontiguousarray(frame_ids, dtype=np.uint64)
            keep.append(fi)
            a.frame_ids = C.ptr(fi, C.U64)
        a.frame_id0 = int(frame_id0)
        if bits is not None:
            b = np.ascontiguousarray(bits, dtype=np.uint8)
            keep.append(b)
            a.bits = C.ptr(b, C.U8)
            a.bits_stride = 0 if bits_broadcast else self.n_bits
        if phases is not None:
            ph = np.ascontiguousarray(phases, dtype=np.float64)
            keep.append(ph)
            a.phases = C.ptr(ph, C.F64)
            a.phases_stride = 0 if phases_broadcast else ph.size // B
        if noise is not None:
            z = np.ascontiguousarray(noise, dtype=np.float64)
            keep.append(z)
            a.noise = C.ptr(z, C.F64)
            a.noise_stride = 0 if noise_broadcast else z.size // B
        if link_noise is not None:
            lz = np.ascontiguousarray(link_noise, dtype=np.float64)
            keep.append(lz)
            a.link_noise = C.ptr(lz, C.F64)
            a.link_noise_stride = 0 if link_broadcast else lz.size // B
        if link_h is not None:
            lh = np.ascontiguousarray(link_h, dtype=np.float64)
            keep.append(lh)
            a.link_h = C.ptr(lh, C.F64)
            a.link_h_stride = 0 if link_broadcast else lh.size // B
        counts = np.zeros((max(1, n_snr), 4), dtype=np.uint64)
        a.counts = C.ptr(counts, C.U64)
        out = RunResult(counts=counts)
        ferr = np.zeros(B, dtype=np.uint32)
        a.frame_errors = C.ptr(ferr, C.U32)
        out['frame_errors'] = ferr
        if self.coded:
            crc = np.zeros(B, dtype=np.uint8)
            a.frame_crc_ok = C.ptr(crc, C.U8)
            out['crc_ok'] = crc
        a.stages = int(stages)
        cdt, rdt = self.cdt, self.rdt
        if in_signal is not None:
            xs = np.ascontiguousarray(in_signal, dtype=cdt).reshape(-1, self.L)
            keep.append(xs)
            a.in_signal = xs.ctypes.data
            a.in_signal_stride = 0 if xs.shape[0] == 1 else 2 * self.L
        shapes = {
            'signal_tx': ((B, self.L), cdt, 'cap_signal_tx', None),
            'signal_rx': ((B, self.num_rx, self.L), cdt, 'cap_signal_rx', None),
            'data_syms': ((B, self.n_sym * self.Nd), cdt, 'cap_data_syms', None),
            'H': ((B, self.num_rx, self.n_grp, self.N), cdt, 'cap_H', None),
            'pilot_stats': ((B, self.num_rx, self.n_grp, 2), rdt, 'cap_pilot_stats', None),
            'bits_rx': ((B, self.n_bits), np.uint8, 'cap_bits_rx', C.U8),
            'llr': ((B, self.n_re_bits), rdt, 'cap_llr', None),
            'noise_power': ((B, self.num_rx), rdt, 'cap_noise_power', None),
            'tx_syms': ((B, self.n_sym * self.Nd), cdt, 'cap_tx_syms', None),
        }
        if self.mimo:
            shapes.update({
                'signal_tx': ((B, self.num_tx, self.L), cdt, 'cap_signal_tx', None),
                'data_syms': ((B, self.n_sym * self.res), cdt, 'cap_data_syms', None),
                'H': ((B, self.num_rx, self.n_est, self.num_tx, self.n_dsc), cdt, 'cap_H', None),
                'link_stats': ((B, self.num_rx, self.num_tx, 4), rdt, 'cap_link_stats', None)})
            shapes.pop('pilot_stats')
            shapes.pop('tx_syms')
        if self.bf:
            shapes.update({'H': ((B, self.num_rx, self.num_tx), cdt, 'cap_H', None),
                           'pmi': ((B,), np.int32, 'cap_pmi', C.I32),
                           'bf_gain': ((B,), np.float64, 'cap_bf_gain', C.F64)})
            for k in ('pilot_stats', 'tx_syms', 'signal_tx', 'signal_rx', 'llr', 'noise_power'):
                shapes.pop(k)
        for name in capture:
            shp, dt, field, ct = shapes[name]
            arr = np.zeros(shp, dtype=dt)
            # void* fields take the address; typed fields a ctypes pointer
            setattr(a, field, arr.ctypes.data if ct is None else C.ptr(arr, ct))
            out[name] = arr
        return a, out, keep

    # ------------------------------------------------------------------
    def timing(self, on=True):
        C.check(C.load().lte_timing_enable(self.h, 1 if on else 0))

    def timing_reset(self):
        C.check(C.load().lte_timing_reset(self.h))

    def timing_read(self):
        names = ctypes.create_string_buffer(512)
        ms = np.zeros(32, dtype=np.float64)
        nl = np.zeros(32, dtype=np.int64)
        n = C.check(C.load().lte_timing_read(self.h, names, 512, C.ptr(ms, C.F64), C.ptr(nl, C.c_i64), 32))
        keys = names.value.decode().split(',')
        return {k: (float(ms[i]), int(nl[i])) for i, k in enumerate(keys[:n])}


_CACHE: "OrderedDict[tuple, Plan]" = OrderedDict()
_CACHE_MAX = 8


def plan_key(**kw):
    """get_plan's cache key for these Plan keywords, and the keywords with their
    defaults resolved (no device call)."""
    kw['precision'] = C.precision_of(kw.get('precision'))   # resolved now: part of the cache key
    kw['early_stop'] = bool(kw.get('early_stop', False))   # likewise: an early-stop plan is never a fixed one
    # likewise the re-packing boundary (True and its default are one plan)
    kw['repack'] = repack_boundary(kw.get('repack'), kw['early_stop'], kw.get('turbo_iters', 8))
    hq = kw.get('harq')   # likewise, as a sorted tuple of its settings (None: a plain plan)
    kw['harq'] = None if hq is None else tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, np.ndarray)) else v)
                                                      for k, v in dict(hq).items()))
    kw['turbo_scale'] = turbo_scale_value(kw.get('turbo_scale'))   # likewise (None and 1 are one plan)
    kw['harq_repack'] = bool(kw.get('harq_repack', False))   # likewise: a re-packing plan is never a plain HARQ one
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in kw.items()))
    return key, kw


def get_plan(**kw):
    key, kw = plan_key(**kw)
    p = _CACHE.get(key)
    if p is None:
        p = Plan(**dict(kw, harq=None if kw['harq'] is None else dict(kw['harq'])))
        _CACHE[key] = p
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    else:
        _CACHE.move_to_end(key)
    return p


def path_diff(a, b):
    """The fields in which two runs' kernel paths (RunResult.path) differ."""
    return {k for k in set(a) | set(b) if a.get(k) != b.get(k)}


def clear_cache():
    _CACHE.clear()
