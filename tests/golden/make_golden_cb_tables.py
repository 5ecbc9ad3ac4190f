"""Code-block tables from the REFERENCE (/root/reference, survey container
only): the tables the channel-coding chain is built on, for every legal code
block size.  Output tests/golden/golden_cb_tables.json (+ _manifest.json).
Data only: table rows and recorded results, no reference source.

  * qpp: the 188 (K, f1, f2) rows of QPP_INTERLEAVER_PARAMS
    (turbo_encoder.py:34-73), in ascending K
  * sizes: TURBO_INTERLEAVER_SIZES (segmentation.py:32-51)
  * seg_info: get_segmentation_info(B) (segmentation.py:362-420) as
    [B, num_blocks, block_sizes, total_coded_bits] for a boundary list of B:
      - K - 1, K, K + 1 for each of the 188 sizes (single block: filler 1, 0
        and the most the next size takes; 6145 is the first two-block B)
      - for C = 2..13 code blocks: the smallest and the largest B that give C
        blocks, and the B nearest the middle of that range whose two block
        sizes differ (K- != K+)

usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cb_tables.py
The output is a pure function of the reference: a second run is byte-identical.
"""
import hashlib
import json
import os
import sys

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
Z, L = 6144, 24


def boundary_sizes(sizes, info):
    bs = set()
    for K in sizes:
        bs.update(b for b in (K - 1, K, K + 1) if b >= 1)
    bs.update((Z, Z + 1))
    for Cn in range(2, 14):
        lo, hi = max(Z, (Cn - 1) * (Z - L)) + 1, Cn * (Z - L)   # B > Z and ceil(B / (Z - L)) == Cn
        assert info(lo)['num_blocks'] == Cn == info(hi)['num_blocks'] and info(lo - 1)['num_blocks'] == Cn - 1
        bs.update((lo, hi))
        mid = (lo + hi) // 2
        for d in range(hi - lo):                             # nearest the middle with two sizes
            for b in (mid + d, mid - d):
                if lo <= b <= hi and len(set(info(b)['block_sizes'])) == 2:
                    bs.add(b)
                    break
            else:
                continue
            break
        else:
            raise SystemExit(f'no B with K- != K+ for C = {Cn}')
    return sorted(bs)


def main():
    if not os.path.isdir(REF):
        sys.exit('needs the reference at /root/reference (survey container only)')
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from core.channel_coding import segmentation, turbo_encoder
    sizes = [int(k) for k in segmentation.TURBO_INTERLEAVER_SIZES]
    qpp = [[int(K), int(f1), int(f2)] for K, (f1, f2) in sorted(turbo_encoder.QPP_INTERLEAVER_PARAMS.items())]
    info = segmentation.get_segmentation_info
    seg = []
    for B in boundary_sizes(sizes, info):
        r = info(B)
        seg.append([B, int(r['num_blocks']), [int(k) for k in r['block_sizes']], int(r['total_coded_bits'])])
    G = {'qpp': qpp, 'sizes': sizes, 'seg_info': seg}
    # one table row per line: a diff of the fixture shows the row that moved
    lines = ['{']
    for i, key in enumerate(sorted(G)):
        rows = ',\n'.join('  ' + json.dumps(r, separators=(',', ':')) for r in G[key])
        lines.append(f' "{key}": [\n{rows}\n ]' + (',' if i + 1 < len(G) else ''))
    lines.append('}')
    text = '\n'.join(lines) + '\n'
    assert json.loads(text) == G
    path = os.path.join(OUT, 'golden_cb_tables.json')
    with open(path, 'w') as f:
        f.write(text)
    man = {'generated_by': 'tests/golden/make_golden_cb_tables.py (reference snapshot 2026-02-13)',
           'sha256': hashlib.sha256(text.encode()).hexdigest(),
           'rows': {k: len(v) for k, v in G.items()}}
    with open(os.path.join(OUT, 'golden_cb_tables_manifest.json'), 'w') as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote golden_cb_tables.json ({len(text)} bytes): ' + ', '.join(f'{k} {len(v)}' for k, v in G.items()))


if __name__ == '__main__':
    main()
