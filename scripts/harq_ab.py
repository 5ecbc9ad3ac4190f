#!/usr/bin/env python3
"""HARQ on the config-2 numerology (20 MHz, 64-QAM, Rayleigh Pedestrian A, TB
27 760, 8 iterations, float64): what a retransmission round costs and what the
decoder's group skip saves.  One call is the 0:2:30 dB grid in run_grid order
(SNR-major frame ids, --frames / 16 trials per point), so most 64-frame decoder
groups hold one SNR.  Two budgets: coded_bits = 0 (3K + 12 per code block, rate
about 1/3) and --coded-bits (default 46 308: rate 0.6).  Timed with Plan.timing
(HIP events around each launch), every leg interleaved on one device.

  1. per round: every kernel slot's milliseconds, the frames still active
     before the round and the decoder groups skipped in it
  2. per round: the `turbo` slot with LTE_HARQ_SKIP 1 against 0, alternated,
     with the spread over the repeats
  3. round 0 of the HARQ plan with coded_bits = 0 against a plain coded plan,
     whole-run milliseconds (the sum of the slots), alternated

One JSON object is written to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ofdm-lte_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

TB, ITERS, SEED, MAX_TX, RV = 27760, 8, 0x5EED, 4, (0, 2, 3, 1)
SNRS = np.arange(0.0, 31.0, 2.0)


def make_plan(F, harq):
    import lte_phy
    from lte_phy import _capi as C
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=20.0, modulation='64-QAM'), channel_type='rayleigh_mp',
                                itu_profile='Pedestrian_A', velocity_kmh=0.0, precision='f64')
    return sim._plan(C.CHAIN_CODED, 0, TB, max_frames=F, iters=ITERS, harq=harq)


def grid_args(F):
    T = F // len(SNRS)
    ids = np.arange(len(SNRS) * T, dtype=np.uint64)
    si = (ids // np.uint64(T)).astype(np.int32)
    return SNRS[si], dict(snr_index=si, n_snr=len(SNRS), seed=SEED, frame_ids=ids)


def timed(plan, snr, kw):
    plan.timing_reset()
    plan.timing(True)
    r = plan.run(snr, **kw)
    tim = plan.timing_read()
    plan.timing(False)
    return {k: v[0] for k, v in tim.items() if v[1]}, r


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {'min': float(x.min()), 'median': float(np.median(x)), 'max': float(x.max()), 'runs': [float(v) for v in x]}


def process(plan, snr, kw, skip):
    """One HARQ process, every round run (no early exit): per round the slots,
    the frames active before it and the groups skipped."""
    os.environ['LTE_HARQ_SKIP'] = '1' if skip else '0'
    rounds, active = [], len(snr)
    for t in range(MAX_TX):
        plan.harq_round(t)
        tim, r = timed(plan, snr, kw)
        rounds.append({'round': t, 'rv': RV[t], 'active_before': int(active),
                       'groups_skipped': r['harq_info']['skipped'], 'ms': tim, 'total_ms': float(sum(tim.values())),
                       'turbo_ms': float(tim.get('turbo', 0.0)), 'path': r.path})
        active = int(np.sum(r['crc_ok'] == 0))
    return rounds, r


def budget(F, G, reps):
    from lte_phy import engine
    plan = make_plan(F, dict(max_tx=MAX_TX, rv_seq=RV, coded_bits=G))
    snr, kw = grid_args(F)
    process(plan, snr, kw, True)                                    # warm-up
    on, off, last = [], [], None
    for _ in range(reps):                                           # alternated
        a, last = process(plan, snr, kw, True)
        b, r_off = process(plan, snr, kw, False)
        on.append(a)
        off.append(b)
        assert np.array_equal(last['tx_used'], r_off['tx_used']) and np.array_equal(last['crc_ok'], r_off['crc_ok'])
    hist = np.bincount(np.where(last['crc_ok'] != 0, last['tx_used'], 0), minlength=MAX_TX + 1)
    out = {'coded_bits': plan.coded_bits, 'code_rate': (TB + 24) / plan.coded_bits, 'n_sym': plan.n_sym,
           'frames': len(snr), 'groups': -(-len(snr) // 64), 'tx_hist_never_1_2_3_4': hist.tolist(),
           'rounds': on[-1],
           'turbo_skip_vs_no_skip': [
               {'round': t, 'groups_skipped': on[-1][t]['groups_skipped'],
                'skip_ms': spread([p[t]['turbo_ms'] for p in on]),
                'no_skip_ms': spread([p[t]['turbo_ms'] for p in off]),
                'ratio_median': float(np.median([p[t]['turbo_ms'] for p in on]) /
                                      np.median([p[t]['turbo_ms'] for p in off]))}
               for t in range(MAX_TX)]}
    del plan
    engine.clear_cache()
    return out


def round0_vs_plain(F, reps):
    from lte_phy import engine
    hq = make_plan(F, dict(max_tx=MAX_TX, rv_seq=RV, coded_bits=0))
    plain = make_plan(F, None)
    snr, kw = grid_args(F)
    timed(hq, snr, kw), timed(plain, snr, kw)
    t_hq, t_pl, s_hq, s_pl = [], [], None, None
    for _ in range(reps):
        s_hq, a = timed(hq, snr, kw)
        s_pl, b = timed(plain, snr, kw)
        t_hq.append(sum(s_hq.values()))
        t_pl.append(sum(s_pl.values()))
        assert np.array_equal(a['counts'], b['counts'])
    h, q = spread(t_hq), spread(t_pl)
    out = {'frames': len(snr), 'harq_round0_ms': h, 'plain_ms': q, 'harq_round0_slots_ms': s_hq, 'plain_slots_ms': s_pl,
           'ratio_median': h['median'] / q['median'],
           'spreads_overlap': bool(h['min'] <= q['max'] and q['min'] <= h['max'])}
    del hq, plain
    engine.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=65536, help='frames per call (a multiple of 16: the SNR grid)')
    ap.add_argument('--coded-bits', type=int, default=46308, help='the punctured budget (rate (TB + 24) / coded bits)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'harq_ab.json'))
    args = ap.parse_args()
    F = args.frames - args.frames % len(SNRS)
    res = {'config': {'bandwidth_mhz': 20.0, 'modulation': '64-QAM', 'channel': 'rayleigh_mp Pedestrian_A', 'tb': TB,
                      'turbo_iters': ITERS, 'snr_db': SNRS.tolist(), 'frames_per_call': F, 'max_tx': MAX_TX,
                      'rv_seq': list(RV), 'precision': 'f64', 'reps': args.reps},
           'budgets': [budget(F, G, args.reps) for G in (args.coded_bits, 0)],
           # two plans side by side: half the frames each
           'round0_vs_plain': round0_vs_plain(F // 2 - (F // 2) % len(SNRS), args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    brief = {'budgets': [{k: b[k] for k in ('coded_bits', 'tx_hist_never_1_2_3_4')} |
                         {'turbo': [(x['round'], x['groups_skipped'], round(x['skip_ms']['median'], 2),
                                     round(x['no_skip_ms']['median'], 2)) for x in b['turbo_skip_vs_no_skip']],
                          'round_total_ms': [round(x['total_ms'], 2) for x in b['rounds']]} for b in res['budgets']],
             'round0_vs_plain': {k: res['round0_vs_plain'][k] for k in ('harq_round0_ms', 'plain_ms', 'ratio_median')}}
    print(json.dumps(brief))


if __name__ == '__main__':
    main()
