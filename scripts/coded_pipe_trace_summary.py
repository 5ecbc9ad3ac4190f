#!/usr/bin/env python3
"""Timeline summary of a rocprofv3 --kernel-trace CSV of bench.py (config 2):
the last step's kernel launches in start order (queue, start and end relative
to the step's first kernel, duration), then what the coded SISO pipeline is
judged by -- how much of the front-end kernels' time lies inside the span of
the decoder launches, and how much the decoder launches overlap one another.

    python scripts/coded_pipe_trace_summary.py <kernel_trace.csv> [--step-kernel k_payload] > summary.md
"""
import argparse
import csv
import re

FRONT = ('k_fading', 'k_ofdm_tx', 'k_chan_fix', 'k_npow', 'k_rx_frame', 'k_dematch')


def short(name):
    m = re.search(r'(k_[a-z0-9_]+|__amd_rocclr_[A-Za-z]+)', name)
    return m.group(1) if m else name[:40]


def overlap(a, b):
    return max(0, min(a[1], b[1]) - max(a[0], b[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('trace')
    ap.add_argument('--step-kernel', default='k_payload', help='the kernel that opens a step')
    args = ap.parse_args()
    rows = []
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name']), r['Queue_Id']))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if r[2] == args.step_kernel]
    if not starts:
        raise SystemExit(f'no {args.step_kernel} launch in the trace')
    step = rows[starts[-1]:]
    step = [r for r in step if not r[2].startswith('__amd')]
    t0 = step[0][0]
    print(f'# last step of {len(starts)}: {len(step)} kernel launches\n')
    print('| # | kernel | queue | start ms | end ms | ms |')
    print('|---|---|---|---|---|---|')
    for i, (s, e, n, q) in enumerate(step):
        print(f'| {i} | {n} | {q} | {(s - t0) / 1e6:.2f} | {(e - t0) / 1e6:.2f} | {(e - s) / 1e6:.2f} |')
    dec = [(s, e) for s, e, n, q in step if n.startswith('k_turbo')]
    fe = [(s, e, n) for s, e, n, q in step if n.startswith(FRONT)]
    span = (min(s for s, _ in dec), max(e for _, e in dec))
    fe_ns = sum(e - s for s, e, _ in fe)
    fe_in = sum(overlap((s, e), span) for s, e, _ in fe)
    dd = sum(overlap(dec[i], dec[j]) for i in range(len(dec)) for j in range(i + 1, len(dec)))
    end = max(e for _, e, _, _ in step)
    print(f'\n- step, first kernel start to last kernel end: {(end - t0) / 1e6:.2f} ms')
    print(f'- decoder launches: {len(dec)}, their span {(span[1] - span[0]) / 1e6:.2f} ms, '
          f'summed durations {sum(e - s for s, e in dec) / 1e6:.2f} ms, pairwise overlap {dd / 1e6:.2f} ms')
    print(f'- front-end kernels (fading .. dematch): {len(fe)} launches, {fe_ns / 1e6:.2f} ms summed, '
          f'{fe_in / 1e6:.2f} ms of it inside the decoder span')


if __name__ == '__main__':
    main()
