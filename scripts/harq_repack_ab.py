#!/usr/bin/env python3
"""HARQ re-packing of the unacknowledged frames (lte_plan_set_harq_repack) on
scripts/harq_ab.py's workload: config-2 numerology, float64, 8 iterations, the
0:2:30 dB grid in run_grid order, coded_bits = --coded-bits (default 46 308:
rate 0.6) and 0.  One plan per budget; a process with the setting on and one
with it off alternate --reps times (Plan.timing: HIP events around each
launch), every round run.

Per round and budget: the `turbo` and `harq` slots on and off with the spread
over the repeats, M, A, P, cap and the state, the decoder groups per slot
without and with re-packing (lte_harq_repack_rule on the round before's
crc_ok), the time ratio next to the waves ratio, and the bytes the gather
moves.  The latched results of both processes are compared.

--parent ROOT: a tree of the parent commit with its own library built.  Its
scripts/harq_ab.py then runs in a child process between the repeats (--reps 1
each), and its rounds (the skip on: this build's setting off) go to the same
file, next to this build's setting-off rounds.

One JSON object is written to --out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ofdm-lte_amd'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

import harq_ab as AB   # noqa: E402  (the workload and the timing method)


def process(plan, snr, kw, repack):
    """One HARQ process, every round run: per round the slots, the rule's
    counts on the round before's acknowledgements and what the plan reports."""
    from lte_phy import _capi as C
    os.environ['LTE_HARQ_SKIP'] = '1'
    plan.set_harq_repack(repack)
    cap = plan.harq_repack_info()['cap']
    rounds, prev = [], None
    for t in range(AB.MAX_TX):
        plan.harq_round(t)
        tim, r = AB.timed(plan, snr, kw)
        rule = C.harq_repack_rule(prev, cap) if prev is not None else None
        rounds.append({'round': t, 'rv': AB.RV[t], 'groups_skipped': r['harq_info']['skipped'],
                       'turbo_ms': float(tim.get('turbo', 0.0)), 'harq_ms': float(tim.get('harq', 0.0)),
                       'total_ms': float(sum(tim.values())), 'rule': rule, 'info': r.get('harq_repack_info'),
                       'path': r.path})
        prev = r['crc_ok'].copy()
    return rounds, r


def gather_bytes(plan, A, P):
    """Bytes the gather reads and writes for A frames in P packed groups: the 3K + 12
    input rows of every code block slot, 8 bytes each (one 64-byte sector per element read)."""
    from lte_phy import _capi as C
    K, E = np.zeros(32, dtype=np.int32), np.zeros(32, dtype=np.int32)
    n = C.check(C.load().lte_harq_code_block_bits(AB.TB, 6, 0, C.ptr(K, C.I32), C.ptr(E, C.I32), 32))
    rows = int(sum(3 * int(k) + 12 for k in K[:n]))
    return {'rows': rows, 'read_useful': rows * A * 8, 'read_sectors': rows * A * 64, 'written': rows * P * 64 * 8}


def budget(F, G, reps, between):
    from lte_phy import engine
    plan = AB.make_plan(F, dict(max_tx=AB.MAX_TX, rv_seq=AB.RV, coded_bits=G))
    snr, kw = AB.grid_args(F)
    process(plan, snr, kw, True)                                    # warm-up (allocates the packed arrays)
    process(plan, snr, kw, False)
    on, off = [], []
    for i in range(reps):                                           # alternated
        a, r_on = process(plan, snr, kw, True)
        b, r_off = process(plan, snr, kw, False)
        on.append(a)
        off.append(b)
        for k in ('tx_used', 'crc_ok', 'frame_errors', 'counts'):
            assert np.array_equal(r_on[k], r_off[k]), k
        between(i)
    med = lambda runs, t, k: float(np.median([p[t][k] for p in runs]))
    rounds = []
    for t in range(AB.MAX_TX):
        last = on[-1][t]
        row = {'round': t, 'groups_skipped': last['groups_skipped'], 'info': last['info'], 'rule': last['rule'],
               'turbo_on_ms': AB.spread([p[t]['turbo_ms'] for p in on]),
               'turbo_off_ms': AB.spread([p[t]['turbo_ms'] for p in off]),
               'harq_on_ms': AB.spread([p[t]['harq_ms'] for p in on]),
               'harq_off_ms': AB.spread([p[t]['harq_ms'] for p in off]),
               'total_on_ms': AB.spread([p[t]['total_ms'] for p in on]),
               'total_off_ms': AB.spread([p[t]['total_ms'] for p in off])}
        if med(off, t, 'turbo_ms') > 0:
            row['turbo_time_ratio'] = med(on, t, 'turbo_ms') / med(off, t, 'turbo_ms')
        if last['rule'] and last['rule']['waves_off']:
            row['waves_ratio'] = last['rule']['waves_on'] / last['rule']['waves_off']
        if last['info'] and last['info']['state'] == 'packed':
            row['gather_bytes'] = gather_bytes(plan, last['info']['A'], last['info']['P'])
        rounds.append(row)
    out = {'coded_bits': plan.coded_bits, 'code_rate': (AB.TB + 24) / plan.coded_bits, 'frames': len(snr),
           'groups': -(-len(snr) // 64), 'rounds': rounds}
    del plan
    engine.clear_cache()
    return out


def run_parent(root, frames, coded_bits):
    """The parent tree's scripts/harq_ab.py (--reps 1) in a child process on its own package and library."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'parent.json')
        env = dict(os.environ)
        env.pop('LTE_HARQ_SKIP', None)
        env['LTE_HIP_LIB'] = os.path.join(root, 'ofdm-lte_amd', 'lte_phy', 'liblte_hip.so')
        subprocess.run([sys.executable, os.path.join(root, 'scripts', 'harq_ab.py'), '--frames', str(frames),
                        '--coded-bits', str(coded_bits), '--reps', '1', '--out', out], env=env, check=True,
                       stdout=subprocess.DEVNULL)
        res = json.load(open(out))
    return [{'coded_bits': b['coded_bits'],
             'rounds': [{'round': r['round'], 'groups_skipped': r['groups_skipped'], 'turbo_ms': r['turbo_ms'],
                         'harq_ms': r['ms'].get('harq', 0.0), 'total_ms': r['total_ms']} for r in b['rounds']]}
            for b in res['budgets']]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=65536, help='frames per call (a multiple of 16: the SNR grid)')
    ap.add_argument('--coded-bits', type=int, default=46308, help='the punctured budget (rate (TB + 24) / coded bits)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--parent', default=None, help="a built tree of the parent commit (its scripts/harq_ab.py runs)")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'harq_repack_ab.json'))
    args = ap.parse_args()
    F = args.frames - args.frames % len(AB.SNRS)
    parent = []

    def between(i):
        if args.parent:
            parent.append(run_parent(args.parent, F, args.coded_bits))

    res = {'config': {'bandwidth_mhz': 20.0, 'modulation': '64-QAM', 'channel': 'rayleigh_mp Pedestrian_A', 'tb': AB.TB,
                      'turbo_iters': AB.ITERS, 'snr_db': AB.SNRS.tolist(), 'frames_per_call': F, 'max_tx': AB.MAX_TX,
                      'rv_seq': list(AB.RV), 'precision': 'f64', 'reps': args.reps},
           'budgets': [budget(F, G, args.reps, between if G else lambda i: None) for G in (args.coded_bits, 0)]}
    if parent:
        # per budget and round the parent's runs (one per repeat) beside this build's setting-off runs
        res['parent'] = []
        for bi, b in enumerate(res['budgets']):
            rows = []
            for t in range(AB.MAX_TX):
                pt = [run[bi]['rounds'][t] for run in parent]
                rows.append({'round': t, 'parent_turbo_ms': AB.spread([x['turbo_ms'] for x in pt]),
                             'parent_total_ms': AB.spread([x['total_ms'] for x in pt]),
                             'off_turbo_ms': b['rounds'][t]['turbo_off_ms'], 'off_total_ms': b['rounds'][t]['total_off_ms']})
            res['parent'].append({'coded_bits': b['coded_bits'], 'rounds': rows})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    brief = [{'coded_bits': b['coded_bits'],
              'rounds': [(r['round'], r['info']['state'], r['info']['M'], r['info']['A'], r['info']['P'],
                          round(r['turbo_on_ms']['median'], 2), round(r['turbo_off_ms']['median'], 2),
                          round(r.get('turbo_time_ratio', 0), 3), round(r.get('waves_ratio', 0), 3))
                         for r in b['rounds']]} for b in res['budgets']]
    print(json.dumps(brief))


if __name__ == '__main__':
    main()
