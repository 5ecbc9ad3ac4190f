#!/usr/bin/env python3
"""A/B of the turbo decoders' extrinsic scaling (scaled max-log-MAP, scale 0.75)
on the config-2 plan (20 MHz, 64-QAM, Rayleigh Pedestrian A, TB 27 760, 8
iterations).

Three measurements on one device:

  1. time, fixed decoder: the `turbo` slot of Plan.timing (HIP events around
     the decoder launch) for one plan whose scale is switched between runs --
     unscaled / 0.75 / unscaled, alternated --repeats times, float64 and
     float32, Philox mode, frames 0..F-1 of one SNR point.  The unscaled runs
     launch k_turbo64 / k_turbo, the same kernels as before the scaled twins
     existed (scripts/kcmp.py), so they are the yardstick of the same session.
  2. time, early-stop decoder at --es-snr (22 dB) with and without repack=1, the
     same alternation.  The scaled decode stops at other iterations than the
     unscaled one, so next to the times stand the mean n* of both.
  3. BLER: run_grid(coded=True) at the same numerology over --bler-snrs at scale
     1 and 0.75, --trials frames per SNR point; the SNR at which each curve
     crosses BLER 0.1 (log-linear interpolation) and the shift.  --bler-channel
     awgn runs the curves without fading (each frame of config 2's channel has
     one fading state, so its BLER curve is set by the fades, not by the
     decoder's waterfall).

F is the largest power of two up to --frames that fits on the device.  One JSON
line per measurement is appended to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ofdm-lte_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

TB, ITERS, SEED, SCALE = 27760, 8, 0x5EED, 0.75


def simulator(prec, channel='rayleigh_mp'):
    import lte_phy
    return lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=20.0, modulation='64-QAM'), channel_type=channel,
                                 itu_profile='Pedestrian_A', velocity_kmh=0.0, precision=prec)


def make_plan(prec, F, early_stop=False):
    """(F, plan) at the largest power of two <= F that fits."""
    from lte_phy import _capi as C
    from lte_phy import engine
    while F >= 64:
        try:
            return F, simulator(prec)._plan(C.CHAIN_CODED, 0, TB, max_frames=F, iters=ITERS, early_stop=early_stop)
        except (RuntimeError, MemoryError) as e:
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
    ms = plan.timing_read()['turbo'][0]
    plan.timing(False)
    return ms, r


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {'min': float(x.min()), 'median': float(np.median(x)), 'max': float(x.max()), 'runs': [float(v) for v in x]}


def alternate(plan, snr, F, repeats):
    """unscaled / scaled / unscaled, `repeats` times, after a warm-up of both."""
    t = {'unscaled': [], 'scaled': []}
    last = {}
    for s in (None, SCALE):
        plan.set_turbo_scale(s)
        turbo_ms(plan, snr, F)
    for _ in range(repeats):
        for name, s in (('unscaled', None), ('scaled', SCALE), ('unscaled', None)):
            plan.set_turbo_scale(s)
            ms, last[name] = turbo_ms(plan, snr, F)
            t[name].append(ms)
    plan.set_turbo_scale(None)
    u, c = spread(t['unscaled']), spread(t['scaled'])
    # the margin the scaled slot is expected inside: the unscaled repeats' spread plus 2 %
    margin = (u['max'] - u['min']) / u['median'] + 0.02
    line = {'unscaled_ms': u, 'scaled_ms': c, 'ratio_median': c['median'] / u['median'],
            'margin': margin, 'within_margin': bool(c['median'] <= u['median'] * (1 + margin)),
            'bler_unscaled': float(last['unscaled']['counts'][0, 2]) / float(last['unscaled']['counts'][0, 3]),
            'bler_scaled': float(last['scaled']['counts'][0, 2]) / float(last['scaled']['counts'][0, 3])}
    for name in ('unscaled', 'scaled'):
        if 'turbo_iters_used' in last[name]:
            line['mean_n_star_' + name] = float(last[name]['turbo_iters_used'].mean())
    line['path_scaled'] = last['scaled'].path
    return line


def timing(args, out):
    from lte_phy import engine
    for prec in args.precisions:
        F, plan = make_plan(prec, args.frames)
        out(dict(measurement='fixed_scaled_vs_unscaled', precision=prec, frames=F, snr_db=args.snr, iters=ITERS,
                 scale=SCALE, **alternate(plan, args.snr, F, args.repeats)))
        del plan
        engine.clear_cache()
        F, plan = make_plan(prec, args.frames, early_stop=True)
        for repack in (0, 1):
            plan.set_repack(repack)
            out(dict(measurement='early_stop_scaled_vs_unscaled', precision=prec, frames=F, snr_db=args.es_snr,
                     iters=ITERS, scale=SCALE, repack=repack, **alternate(plan, args.es_snr, F, args.repeats)))
        del plan
        engine.clear_cache()


def crossing(snrs, bler, level=0.1):
    """SNR at which a falling curve crosses `level`, log-linear between its neighbours (None: it does not)."""
    for i in range(len(snrs) - 1):
        a, b = bler[i], bler[i + 1]
        if a >= level > b and b > 0:
            return float(snrs[i] + (snrs[i + 1] - snrs[i]) * (np.log10(a) - np.log10(level)) / (np.log10(a) - np.log10(b)))
    return None


def bler(args, out):
    snrs = list(args.bler_snrs)
    curves = {}
    for s in (1.0, SCALE):
        sim = simulator(args.bler_precision, args.bler_channel)
        sim.turbo_scale = s
        r = sim.run_grid(snrs, args.trials, seed=SEED, coded=True, frames_per_call=args.bler_frames_per_call)
        curves[s] = r
    x1, xs = (crossing(snrs, curves[s]['bler']) for s in (1.0, SCALE))
    out({'measurement': 'bler_scaled_vs_unscaled', 'channel': args.bler_channel, 'precision': args.bler_precision,
         'trials': args.trials,
         'iters': ITERS, 'scale': SCALE, 'snr_db': snrs,
         'block_errors_unscaled': [int(v) for v in curves[1.0]['block_errors']],
         'block_errors_scaled': [int(v) for v in curves[SCALE]['block_errors']],
         'bler_unscaled': [float(v) for v in curves[1.0]['bler']], 'bler_scaled': [float(v) for v in curves[SCALE]['bler']],
         'ber_unscaled': [float(v) for v in curves[1.0]['ber']], 'ber_scaled': [float(v) for v in curves[SCALE]['ber']],
         'snr_at_bler_0.1_unscaled': x1, 'snr_at_bler_0.1_scaled': xs,
         'shift_db_at_bler_0.1': None if x1 is None or xs is None else x1 - xs})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=3, help='unscaled / scaled / unscaled rounds per leg')
    ap.add_argument('--snr', type=float, default=18.0, help='SNR (dB) of the fixed decoder runs')
    ap.add_argument('--es-snr', type=float, default=22.0, help='SNR (dB) of the early-stop runs')
    ap.add_argument('--precisions', nargs='+', default=['f64', 'f32'], choices=('f64', 'f32'))
    ap.add_argument('--bler-snrs', type=float, nargs='+', default=[float(v) for v in range(16, 25)])
    ap.add_argument('--trials', type=int, default=16384, help='frames per SNR point of the BLER curves')
    ap.add_argument('--bler-frames-per-call', type=int, default=16384)
    ap.add_argument('--bler-channel', default='rayleigh_mp', choices=('rayleigh_mp', 'awgn'),
                    help="channel of the BLER curves (config 2's is rayleigh_mp; awgn: the same numerology without fading)")
    ap.add_argument('--bler-precision', default='f64', choices=('f64', 'f32'))
    ap.add_argument('--skip-timing', action='store_true')
    ap.add_argument('--skip-bler', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'turbo_scale_ab.json'))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def out(line):
        s = json.dumps(line)
        print(s, flush=True)
        with open(args.out, 'a') as f:
            f.write(s + '\n')

    if not args.skip_timing:
        timing(args, out)
    if not args.skip_bler:
        bler(args, out)


if __name__ == '__main__':
    main()
