#!/usr/bin/env python3
"""A/B of re-packing the early-stop turbo decoder's undecided blocks on the
config-2 plan (20 MHz, 64-QAM, Rayleigh Pedestrian A, TB 27 760, 8
iterations), timed with Plan.timing's `turbo` slot (HIP events around the whole
decode: first window, counts, gather, second window, scatter).

Legs, interleaved on one device at every SNR point: the fixed-iteration plan,
the early-stop plan, and that same early-stop plan with the boundary switched
to each of --boundaries (lte_plan_set_early_stop_repack; the packed arrays stay
allocated, so the legs share one set of decoder arrays).  Frames in run_grid
order (ids 0..F-1 of one SNR point).  F is the largest power of two up to
--frames for which the plans of a precision fit on the device.  A warm-up run of
every leg, then --reps timed rounds.  One JSON line per (precision, SNR) is
appended to --out: the spreads, the undecided counts and states of repack_info,
the path strings, and whether each boundary's spread overlaps plain early
stop's.  Every leg's outputs are also compared with plain early stop's (they
must be identical)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from early_stop_ab import ITERS, make_plan, spread, turbo_ms  # noqa: E402  (also puts the package on sys.path)


def plans(prec, F, after):
    """(F, fixed plan, early-stop plan with its packed arrays) at the largest power of two <= F that fits."""
    from lte_phy import engine
    while F >= 64:
        try:
            fx, es = make_plan(prec, F, False), make_plan(prec, F, True)
            es.set_repack(after)      # allocates the packed arrays
            es.set_repack(0)
            return F, fx, es
        except (RuntimeError, MemoryError) as e:
            fx = es = None
            print(f'# {prec}: {F} frames do not fit ({e}); halving', file=sys.stderr)
            engine.clear_cache()
            F //= 2
    raise SystemExit('no frame count fits')


def overlap(a, b):
    return bool(a['min'] <= b['max'] and b['min'] <= a['max'])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=5, help='timed runs per leg')
    ap.add_argument('--precisions', nargs='+', default=['f64', 'f32'], choices=('f64', 'f32'))
    ap.add_argument('--snrs', type=float, nargs='+', default=[0.0, 18.0, 22.0, 26.0, 30.0])
    ap.add_argument('--boundaries', type=int, nargs='+', default=[1, 2, 3])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'early_stop_repack_ab.json'))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    from lte_phy import engine
    for prec in args.precisions:
        F, fx, es = plans(prec, args.frames, args.boundaries[0])
        legs = ['fixed', 'early_stop'] + [f'repack_{a}' for a in args.boundaries]

        def run(leg, snr):
            if leg == 'fixed':
                return turbo_ms(fx, snr, F)
            es.set_repack(int(leg.split('_')[1]) if leg.startswith('repack_') else 0)
            return turbo_ms(es, snr, F)

        for snr in args.snrs:
            res = {leg: run(leg, snr)[1] for leg in legs}                     # warm-up of every leg
            t = {leg: [] for leg in legs}
            for _ in range(args.reps):                                         # interleaved
                for leg in legs:
                    ms, res[leg] = run(leg, snr)
                    t[leg].append(ms)
            plain = res['early_stop']
            used = plain['turbo_iters_used'].astype(np.float64)
            wave_max = used.reshape(F // 64, 64, -1).max(axis=1) if F % 64 == 0 else used[None]
            line = {'measurement': 'early_stop_repack', 'precision': prec, 'frames': F, 'snr_db': snr, 'iters': ITERS,
                    'n_cb': int(used.shape[1]),
                    'bler': float(plain['counts'][0, 2]) / float(plain['counts'][0, 3]),
                    'mean_n_star': float(used.mean()), 'mean_wave_max_n_star': float(wave_max.mean()),
                    'ms': {leg: spread(t[leg]) for leg in legs},
                    'path': {leg: ' '.join(f'{k}={v}' for k, v in res[leg].path.items()) for leg in legs},
                    'repack': {}}
            fixed_med = line['ms']['fixed']['median']
            line['ratio_to_fixed'] = {leg: line['ms'][leg]['median'] / fixed_med for leg in legs}
            for a in args.boundaries:
                r = res[f'repack_{a}']
                same = all(np.array_equal(r[k], plain[k])
                           for k in ('turbo_iters_used', 'counts', 'frame_errors', 'crc_ok'))
                if not same:
                    raise SystemExit(f'{prec} {snr} dB repack={a}: outputs differ from plain early stop')
                line['repack'][str(a)] = dict(r['repack_info'], identical_outputs=same,
                                              spreads_overlap_early_stop=overlap(line['ms'][f'repack_{a}'],
                                                                                 line['ms']['early_stop']))
            s = json.dumps(line)
            print(s, flush=True)
            with open(args.out, 'a') as f:
                f.write(s + '\n')
        del fx, es
        engine.clear_cache()


if __name__ == '__main__':
    main()
