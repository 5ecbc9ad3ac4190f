#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of one translation unit.

    python scripts/kcmp.py OLD.o NEW.o      (host objects or shared libraries)

Prints the kernels present in only one of the two, those whose disassembly
differs and those whose metadata note differs (registers, spills, LDS, scratch,
kernarg size); exits 1 on any difference.  Whole bodies are compared by hash,
with addresses stripped, so the order of the kernels in the code object does
not matter.  A refactor of the host-side launchers must come out clean.
"""
import bisect
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
META = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
        'group_segment_fixed_size', 'private_segment_fixed_size', 'kernarg_segment_size',
        'max_flat_workgroup_size', 'wavefront_size')


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_object(path, tmp, tag):
    """Unbundle the gfx950 code object of a host object / .so (as kres.sh does);
    None for a host-only object (no .hip_fatbin section)."""
    fat, co = os.path.join(tmp, tag + '.fat'), os.path.join(tmp, tag + '.co')
    if '.hip_fatbin' not in tool('llvm-readelf', '-S', '--wide', path):
        return None
    # (without an output file objcopy rewrites its input)
    tool('llvm-objcopy', '--dump-section=.hip_fatbin=' + fat, path, os.path.join(tmp, tag + '.copy'))
    tool('clang-offload-bundler', '--unbundle', '--type=o', '--input=' + fat, '--targets=' + TARGET, '--output=' + co)
    return co


def data_symbols(co):
    """Sorted (address, name, size) of the code object's data symbols (constant tables)."""
    syms = set()
    for line in tool('llvm-readelf', '-s', '--wide', co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == 'OBJECT' and f[6].isdigit():
            syms.add((int(f[1], 16), f[7], int(f[2], 0)))
    return sorted(syms)


def bodies(co):
    """{symbol: hash of its disassembly}, split at the symbol headers.

    Addresses are dropped.  A pc-relative reference to constant data (getpc,
    then an add of a 32-bit literal to the low register) moves with the layout
    of the code object, so its literal is rewritten as table + offset.  The
    same sequence with a target in no table is a long branch inside the kernel
    (the f64 decoders are long enough to need them): its literal is relative
    to the kernel's own code and stays as it is."""
    syms = data_symbols(co)
    out, name, h, pcs = {}, None, None, {}
    for line in tool('llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', co).splitlines():
        m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:$', line)
        if m:
            name, h, pcs = m.group(1), hashlib.sha256(), {}
            out[name] = h
            continue
        if name is None or not line.strip():
            continue
        addr = re.search(r'//\s*([0-9A-Fa-f]+):', line)
        ins = re.sub(r'\s*//.*$', '', line).strip()
        m = re.match(r's_getpc_b64 s\[(\d+):\d+\]$', ins)
        if m and addr:
            pcs['s' + m.group(1)] = int(addr.group(1), 16) + 4   # the pc it returns
        m = re.match(r's_add_u32 (s\d+), (s\d+), (0x[0-9a-f]+)$', ins)
        if m and m.group(1) == m.group(2) and m.group(1) in pcs:
            imm = int(m.group(3), 16)
            target = pcs.pop(m.group(1)) + (imm - (1 << 32) if imm >> 31 else imm)
            i = bisect.bisect_right(syms, (target, '\uffff'))
            if i and target < syms[i - 1][0] + syms[i - 1][2]:
                ins = f's_add_u32 {m.group(1)}, {m.group(2)}, {syms[i - 1][1]}+{target - syms[i - 1][0]}'
        h.update(ins.encode() + b'\n')
    return {k: v.hexdigest() for k, v in out.items()}


def metadata(co):
    """{kernel: {field: value}} from the code object's metadata note."""
    out = {}
    for blk in re.split(r'\n\s+- \.agpr_count', tool('llvm-readelf', '--notes', co))[1:]:
        blk = '.agpr_count' + blk
        m = re.search(r'\.name:\s+(\S+)', blk)
        if m:
            f = {k: re.search(r'\.%s:\s+(\S+)' % k, blk) for k in META}
            out[m.group(1)] = {k: v.group(1) for k, v in f.items() if v}
    return out


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        co = [code_object(p, tmp, t) for p, t in ((old, 'old'), (new, 'new'))]
        body = [bodies(c) if c else {} for c in co]
        meta = [metadata(c) if c else {} for c in co]
    bad = 0
    for tag, a, b in (('only in old', 0, 1), ('only in new', 1, 0)):
        for k in sorted((set(body[a]) | set(meta[a])) - (set(body[b]) | set(meta[b]))):
            print(f'{tag}: {k}')
            bad += 1
    for k in sorted(set(body[0]) & set(body[1])):
        if body[0][k] != body[1][k]:
            print(f'body differs: {k}')
            bad += 1
    for k in sorted(set(meta[0]) & set(meta[1])):
        if meta[0][k] != meta[1][k]:
            d = ' '.join(f'{f}={meta[0][k].get(f)}->{meta[1][k].get(f)}' for f in META
                         if meta[0][k].get(f) != meta[1][k].get(f))
            print(f'metadata differs: {k}: {d}')
            bad += 1
    order = '' if list(body[0]) == list(body[1]) else ', in another order'
    print(f'{os.path.basename(new)}: {len(meta[1])} kernels, {len(body[1])} functions{order}: '
          + ('identical' if not bad else f'{bad} differences'))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
