"""Models of the scaled max-log turbo decoders (a helper, not a conftest).

The definition, in the words of include/lte_phy.h (lte_plan_set_turbo_scale):

A scale s is a number with 0 < s <= 1.  In every decoder-1 and decoder-2
half-iteration the extrinsic is

    e = s * ((L - La) - Ls)

- The two subtractions are as without scaling (turbo_decoder.py:270).
- One further multiply follows, rounded separately in the plan's arithmetic.
- In float32 plans the factor is (float)s.
- The multiply is not contracted into a neighbouring add.
- The decoder rows hold halves: s * ((0.5 L - la) - ls) is exactly half of e,
  so the row convention does not change.
- The a-posteriori L is not scaled.  That covers the final pass and the
  decoder-1 decisions the early-stop kernels pack.
- The inputs Ls, Lp and the HARQ soft rows are not scaled.
- The early-stop rule is unchanged.  D(n) are now the decisions of the scaled
  decode of n iterations.
- Re-packing stays "bit for bit the plan without re-packing".
- s = 1 means no scaling.  It launches the unscaled kernels, with no
  multiply-by-one instance, and every output is bit for bit the unscaled one.

Float64: the turbo_decode loop restated from oracle.bcjr_app and
oracle.qpp_perm (as turbo_decode_logmap in tests/test_gpu_code_blocks.py does
for log-MAP) with the one multiply.  Float32: turbo_scaled_model.c, the
oracle's float32 kernel model restated with the one multiply, built here with
the host compiler.  Both return the decisions after every iteration n = 0 ..
iters of one pass, which is what the early-stop rule needs: D(n) are the signs
of the decoder-1 pass that follows iteration n (the final pass of an
n-iteration decode has exactly its inputs).
"""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
POLYS = {'24A': 0x1864CFB, '24B': 0x1800063}
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        cc = next((shutil.which(c) for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
        if cc is None:
            raise RuntimeError('no host C compiler for tests/turbo_scaled_model.c')
        out = os.path.join(tempfile.mkdtemp(prefix='turbo_scaled_model_'), 'turbo_scaled_model.so')
        subprocess.run([cc, '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-Wall', '-Werror',
                        os.path.join(HERE, 'turbo_scaled_model.c'), '-o', out], check=True)
        lib = ctypes.CDLL(out)
        lib.tsm_decode_f32.restype = None
        lib.tsm_decode_f32.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                       ctypes.c_void_p]
        _LIB = lib
    return _LIB


def decisions_f64(O, llr, K, iters, scale=1.0):
    """D(0) .. D(iters) [iters + 1][K] of one block, llr [3K + 12] float64."""
    llr = np.asarray(llr, dtype=np.float64)
    perm = O.qpp_perm(K)
    z3 = np.zeros(3)
    sy, p1, p2 = llr[0:3 * K:3], llr[1:3 * K:3], llr[2:3 * K:3]
    ls1 = np.concatenate([sy, llr[3 * K:3 * K + 3]])
    lp1 = np.concatenate([p1, llr[3 * K + 3:3 * K + 6]])
    ls2 = np.concatenate([sy[perm], llr[3 * K + 6:3 * K + 9]])
    lp2 = np.concatenate([p2, llr[3 * K + 9:3 * K + 12]])
    s = np.float64(scale)
    e21 = np.zeros(K)
    out = np.zeros((iters + 1, K), dtype=np.uint8)
    for it in range(iters + 1):
        la = np.concatenate([e21, z3])
        app = O.bcjr_app(ls1, lp1, la)
        out[it] = app[:K] < 0
        if it == iters:
            break
        e12 = ((app - la) - ls1)[:K]
        if scale != 1.0:
            e12 = s * e12
        la = np.concatenate([e12[perm], z3])
        e = ((O.bcjr_app(ls2, lp2, la) - la) - ls2)[:K]
        if scale != 1.0:
            e = s * e
        e21 = np.zeros(K)
        e21[perm] = e          # qpp_deinterleave: out[perm[i]] = in[i]
    return out


def decisions_f32(O, llr, K, iters, scale=1.0):
    """D(0) .. D(iters) [iters + 1][K] of one block in the float32 model."""
    L = np.ascontiguousarray(llr, dtype=np.float32)
    assert L.shape == (3 * K + 12,)
    perm = np.ascontiguousarray(O.qpp_perm(K), dtype=np.int32)
    out = np.zeros((iters + 1, K), dtype=np.uint8)
    _lib().tsm_decode_f32(L.ctypes.data, K, iters, perm.ctypes.data, float(scale), out.ctypes.data)
    return out


def decisions(O, llr, K, iters, scale=1.0, f32=False):
    return (decisions_f32 if f32 else decisions_f64)(O, llr, K, iters, scale)


def turbo_decode_scaled(O, llr, K, iters, scale=1.0, f32=False):
    """The fixed decode: D(iters)."""
    return decisions(O, llr, K, iters, scale, f32)[iters]


def rule(O, llr, K, iters, poly, scale=1.0, f32=False, D=None):
    """(D(n*), n*, passed) of one code block under the early-stop rule: n* = the
    first n in 1..iters whose D(n) has CRC-24 remainder zero over all K bits,
    iters if none has (0 for iters = 0)."""
    if D is None:
        D = decisions(O, llr, K, iters, scale, f32)
    for n in range(1, iters + 1):
        if not O.crc_bits(D[n], poly, 24).any():
            return D[n], n, True
    return D[iters], iters, False


def undecided_after(O, D, poly, after):
    """Whether the rule leaves the block undecided after the check of D(after)."""
    return all(O.crc_bits(D[n], poly, 24).any() for n in range(1, after + 1))


def coded_rx_decode(O, L, seg, rm_lens, iters=8, scale=1.0, f32=False, early_stop=False):
    """oracle.coded_rx_decode with these decoders: rate dematch, the scaled
    decode per code block -- fixed, or (early_stop) the rule with gCRC24A for a
    transport block of one code block and gCRC24B for several --,
    desegmentation, the transport block's CRC-24A.  Returns (bits, crc ok, n*
    per block, passed per block)."""
    poly = POLYS['24A'] if len(seg) == 1 else POLYS['24B']
    off, dec, ns, ps = 0, [], [], []
    for (K, F, info, o, crc), E in zip(seg, rm_lens):
        dm = O.rate_dematch(L[off:off + E], K, 0)
        off += E
        if f32:
            dm = dm.astype(np.float32)
        if early_stop:
            d, n, p = rule(O, dm, K, iters, poly, scale, f32)
        else:
            d, n, p = turbo_decode_scaled(O, dm, K, iters, scale, f32), iters, True
        dec.append(d)
        ns.append(n)
        ps.append(p)
    tbc = O.desegment(dec, seg)
    return (tbc[:-24] if len(tbc) >= 24 else tbc), O.check_crc24a(tbc), ns, ps


# ---------------------------------------------------------------------------
# The pools of the GPU stage tests (tests/test_gpu_turbo_scale.py), built as
# stage_pool of tests/test_gpu_early_stop.py builds its own; the conditions on
# them are checked from the models alone in tests/test_turbo_scale_host.py.
ITERS = 8
NCB = 2 * 64 + 3
SCALES = {False: (0.75, 0.5), True: (0.75, 0.6875)}   # f32 -> the scales of the fixed-decoder tests
ES_SCALE = 0.75                                       # the early-stop tests' scale
# K -> (ladder of per-block SNRs in dB, {generator: seed}).  40: two words, the
# last one partial; 48, 56: 6 / 7 sub-windows (56: a remainder against the
# 24-step super-window); 64: whole words; 1056, 6144: many super-windows.
# seed: moved (never a condition) until the pool meets pool_conditions for
# both precisions and every scale
STAGE = {40: (np.linspace(-1.0, 4.0, 47), {'24A': 0, '24B': 0}),
         48: (np.linspace(-1.0, 4.0, 47), {'24A': 1, '24B': 0}),
         56: (np.linspace(-1.0, 4.0, 47), {'24A': 2, '24B': 1}),
         64: (np.linspace(-1.0, 4.0, 47), {'24A': 2, '24B': 0}),
         1056: (np.linspace(1.5, 4.0, 15), {'24A': 2, '24B': 0}),
         6144: (np.linspace(2.5, 3.75, 11), {'24A': 6, '24B': 2})}
_LLR, _POOL = {}, {}


def stage_llrs(O, K, crc):
    """Distinct blocks of one K: random payload + CRC-24 (generator `crc`),
    turbo-encoded, BPSK LLRs 2y / s2 with y = 1 - 2c + sqrt(s2) randn at the
    block's own SNR, and last the all-zero word with strong LLRs (it passes:
    zero-init CRC).  [n][3K + 12] float64."""
    if (K, crc) not in _LLR:
        snrs, seeds = STAGE[K]
        rs = np.random.RandomState(1000 * seeds[crc] + K)
        llr = []
        for snr in snrs:
            p = rs.randint(0, 2, K - 24).astype(np.uint8)
            cb = np.concatenate([p, O.crc_bits(p, POLYS[crc], 24)])
            s2 = 10 ** (-snr / 10)
            y = 1 - 2.0 * O.turbo_encode(cb) + np.sqrt(s2) * rs.randn(3 * K + 12)
            llr.append(2 * y / s2)
        llr.append(np.full(3 * K + 12, 8.0))
        _LLR[(K, crc)] = np.array(llr)
    return _LLR[(K, crc)]


def stage_pool(O, K, crc, f32, scale):
    """(llr [n][3K + 12] in the precision's type, D [n][ITERS + 1][K], n*
    [n], passed [n]) of the pool under the model with this scale."""
    key = (K, crc, f32, float(scale))
    if key not in _POOL:
        llr = stage_llrs(O, K, crc).astype(np.float32 if f32 else np.float64)
        D = np.array([decisions(O, l, K, ITERS, scale, f32) for l in llr])
        res = [rule(O, None, K, ITERS, POLYS[crc], D=d) for d in D]
        _POOL[key] = (llr, D, np.array([r[1] for r in res]), np.array([r[2] for r in res]))
    return _POOL[key]


def stage_lanes(passed):
    """Pool index of each of the NCB lanes: wave 0 every pool block in turn,
    wave 1 the passing ones only, then three more of any kind."""
    n = len(passed)
    ok = np.flatnonzero(passed)
    return np.concatenate([np.arange(64) % n, ok[np.arange(64) % len(ok)], ok[np.arange(3) % len(ok)]])


def mixing(n_star, passed):
    """The `mixing` condition of tests/test_gpu_early_stop.py: lanes 0..63 hold
    at least three stopping iterations, one of them a block that never passes;
    every later lane passes before the last iteration."""
    n_star, passed = np.asarray(n_star), np.asarray(passed)
    return len(set(n_star[:64].tolist())) >= 3 and not passed[:64].all() and passed[64:].all() and \
        n_star[64:].max() < ITERS


def pool_conditions(O, K, crc, f32, scale):
    """The conditions without which a kernel that ignored the scale could pass:
    (blocks whose scaled D(8) differs from the unscaled D(8), blocks whose n*
    differs, `mixing` of the scaled n* over the lanes)."""
    _, D, n_star, passed = stage_pool(O, K, crc, f32, scale)
    _, D1, n1, _ = stage_pool(O, K, crc, f32, 1.0)
    lanes = stage_lanes(passed)
    return (int(np.sum((D[:, ITERS] != D1[:, ITERS]).any(axis=1))), int(np.sum(n_star != n1)),
            bool(mixing(n_star[lanes], passed[lanes])))
