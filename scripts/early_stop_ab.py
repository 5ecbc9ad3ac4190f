#!/usr/bin/env python3
"""A/B of the turbo decoder's CRC early termination on the config-2 plan
(20 MHz, 64-QAM, Rayleigh Pedestrian A, TB 27 760, 8 iterations), timed with
Plan.timing's `turbo` slot (HIP events around the decoder launch).

Two measurements, each interleaved on one device:

  1. early stop on vs off, float64 and float32, Philox mode, frames in
     run_grid order (ids 0..F-1 of one SNR point, so every 64-frame wave shares
     its SNR), at 0 dB (no block passes: the price of the check), at the cliff
     and at 30 dB.  Next to the times: the mean n*, the mean over waves of the
     wave's largest n* (a wave leaves when its last block is done), and the
     half-pass counts (1 + 2 n) / 17 both predict.
  2. the default (fixed-iteration) decoder of this tree vs a library built
     from the parent commit (--parent-lib), each run in a fresh process because
     a process loads one liblte_hip.so (LTE_HIP_LIB).

F is the largest power of two up to --frames for which both plans of a
precision fit on the device.  One JSON line per measurement is appended to
--out."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ofdm-lte_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

TB, ITERS, SEED = 27760, 8, 0x5EED


def make_plan(prec, F, early_stop):
    import lte_phy
    from lte_phy import _capi as C
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=20.0, modulation='64-QAM'), channel_type='rayleigh_mp',
                                itu_profile='Pedestrian_A', velocity_kmh=0.0, precision=prec)
    return sim._plan(C.CHAIN_CODED, 0, TB, max_frames=F, iters=ITERS, early_stop=early_stop)


def plans(prec, F, both=True):
    """(F, fixed plan, early-stop plan) at the largest power of two <= F that fits."""
    from lte_phy import engine
    fx = None
    while F >= 64:
        try:
            fx = make_plan(prec, F, False)
            return F, fx, make_plan(prec, F, True) if both else None
        except (RuntimeError, MemoryError) as e:
            fx = None
            print(f'# {prec}: {F} frames do not fit ({e}); halving', file=sys.stderr)
            engine.clear_cache()
            F //= 2
    raise SystemExit('no frame count fits')


def turbo_ms(plan, snr, F):
    """One run of F frames at one SNR; the decoder slot's milliseconds and the run's result."""
    ids = np.arange(F, dtype=np.uint64)
    plan.timing_reset()
    plan.timing(True)
    r = plan.run(np.full(F, snr), snr_index=np.zeros(F, dtype=np.int32), n_snr=1, seed=SEED, frame_ids=ids)
    ms, launches = plan.timing_read()['turbo']
    plan.timing(False)
    assert launches == 1
    return ms, r


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {'min': float(x.min()), 'median': float(np.median(x)), 'max': float(x.max()), 'runs': [float(v) for v in x]}


def on_off(args, out):
    for prec in args.precisions:
        F, fx, es = plans(prec, args.frames)
        for snr in (args.snrs or (0.0, args.cliff, 30.0)):
            turbo_ms(fx, snr, F), turbo_ms(es, snr, F)      # warm-up of both
            t_fx, t_es = [], []
            for _ in range(args.reps):                      # interleaved
                ms, r_fx = turbo_ms(fx, snr, F)
                t_fx.append(ms)
                ms, r = turbo_ms(es, snr, F)
                t_es.append(ms)
            bler = [float(x['counts'][0, 2]) / float(x['counts'][0, 3]) for x in (r_fx, r)]
            used = r['turbo_iters_used'].astype(np.float64)              # [F, n_cb]
            wave_max = used.reshape(F // 64, 64, -1).max(axis=1) if F % 64 == 0 else used[None]
            line = {'measurement': 'early_stop_on_vs_off', 'precision': prec, 'frames': F, 'snr_db': snr,
                    'iters': ITERS, 'fixed_ms': spread(t_fx), 'early_stop_ms': spread(t_es),
                    'ratio_median': float(np.median(t_es) / np.median(t_fx)),
                    'mean_n_star': float(used.mean()), 'mean_wave_max_n_star': float(wave_max.mean()),
                    'half_pass_ratio_blocks': float((1 + 2 * used.mean()) / (2 * ITERS + 1)),
                    'half_pass_ratio_waves': float((1 + 2 * wave_max.mean()) / (2 * ITERS + 1)),
                    'bler_fixed': bler[0], 'bler_early_stop': bler[1], 'path': r.path}
            out(line)
        del fx, es
        from lte_phy import engine
        engine.clear_cache()


def child(args):
    """Default decoder of whatever library LTE_HIP_LIB names: a line of turbo ms per run."""
    import ctypes
    from lte_phy import _capi as C
    lib = ctypes.CDLL(C.LIB_PATH)
    for name in [n for n in C._SIGS if not hasattr(lib, n)]:     # a library from an older commit
        del C._SIGS[name]
    prec = args.precisions[0]
    F, fx, _ = plans(prec, args.frames, both=False)
    turbo_ms(fx, args.cliff, F)
    print(json.dumps({'frames': F, 'ms': [turbo_ms(fx, args.cliff, F)[0] for _ in range(args.reps)]}))


def branch_vs_parent(args, out):
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        out({'measurement': 'default_branch_vs_parent', 'measured': False,
             'reason': 'no parent library given (--parent-lib)'})
        return
    for prec in args.precisions:
        res = {'branch': [], 'parent': []}
        frames = None
        for rnd in range(args.rounds):                      # interleaved, a fresh process each
            for name in ('parent', 'branch'):
                env = dict(os.environ)
                if name == 'parent':
                    env['LTE_HIP_LIB'] = os.path.abspath(args.parent_lib)
                else:
                    env.pop('LTE_HIP_LIB', None)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--precisions', prec,
                                    '--frames', str(args.frames), '--reps', str(args.reps), '--cliff',
                                    str(args.cliff)], env=env, capture_output=True, text=True, timeout=600)
                if p.returncode:
                    raise SystemExit(f'{name} child failed ({p.returncode}):\n{p.stderr[-2000:]}')
                got = json.loads(p.stdout.strip().splitlines()[-1])
                frames = got['frames']
                res[name] += got['ms']
        b, q = spread(res['branch']), spread(res['parent'])
        out({'measurement': 'default_branch_vs_parent', 'measured': True, 'precision': prec, 'frames': frames,
             'snr_db': args.cliff, 'branch_ms': b, 'parent_ms': q,
             'spreads_overlap': bool(b['min'] <= q['max'] and q['min'] <= b['max'])})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=5, help='timed runs per leg (per process in measurement 2)')
    ap.add_argument('--rounds', type=int, default=3, help='measurement 2: parent / branch process pairs')
    ap.add_argument('--cliff', type=float, default=18.0, help="SNR (dB) of the config's waterfall")
    ap.add_argument('--precisions', nargs='+', default=['f64', 'f32'], choices=('f64', 'f32'))
    ap.add_argument('--parent-lib', default=None, help='liblte_hip.so built from the parent commit')
    ap.add_argument('--snrs', type=float, nargs='+', default=None,
                    help='measurement 1: the SNR points (default: 0, the cliff, 30)')
    ap.add_argument('--skip-on-off', action='store_true')
    ap.add_argument('--skip-parent', action='store_true', help='measurement 1 only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'early_stop_ab.json'))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def out(line):
        s = json.dumps(line)
        print(s, flush=True)
        with open(args.out, 'a') as f:
            f.write(s + '\n')

    if not args.skip_on_off:
        on_off(args, out)
    if not args.skip_parent:
        branch_vs_parent(args, out)


if __name__ == '__main__':
    main()
