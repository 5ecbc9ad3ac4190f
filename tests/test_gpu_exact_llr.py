"""GPU: the turbo decoder kernels, float32 and float64, against the float64
reference (oracle.turbo_decode) on exact-input LLRs.

On the pools of tests/exact_llr_model.py every value of max-log-MAP is a small
multiple of one power of two (tests/test_exact_llr_host.py audits it), so any
correct evaluation order gives the reference's result bit for bit.  The expected
value here is therefore the float64 reference in both precisions, never a
float32 model: a change made to a kernel and to its model together does not
pass.  The pools hold exact ties L == 0, exact zeros (erasures), clipped and
repeated values, and known-answer blocks next to blocks that never converge.

  (1) the pools' conditions, as on the CPU
  (2) the fixed decoders (k_turbo / k_turbo64): 0, 1, 2 and 8 iterations
  (3) the early-stop decoders (k_turbo*_es, and _esw / the re-packing gather
      and scatter with repack = 1, 3), both generators: bits and n* follow the
      rule on the reference's D(1) .. D(8)
  (4) the scaled decoders (k_turbo*_sc, k_turbo*_es_sc) at scale 0.5, which is
      exact on the grid, against turbo_scaled_model.decisions_f64
  (5) the values of one BCJR pass (lte_bcjr_host, lte_bcjr_host64): equal to
      oracle.bcjr_app, ties at exactly 0.0 included
  (6) scale invariance: the decoders' outputs do not change when unquantised
      LLRs are multiplied by 2^+-64 (float32) or 2^+-200 (float64).  This needs
      no reference; an absorbed sentinel, a flushed small value or an
      int-typed intermediate fails it.
k_turbo64_logmap stays out: log1p(exp(.)) is exact on no grid.
"""
import numpy as np
import pytest

import exact_llr_model as X

pytestmark = pytest.mark.gpu

ITERS, SC_ITERS, SC_SCALE, NCB, POLYS = X.ITERS, X.SC_ITERS, X.SC_SCALE, X.NCB, X.POLYS
CASES = [(K, quant, prec) for K in X.KS for quant in X.QUANT for prec in ('f64', 'f32')]


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


@pytest.fixture(scope='module')
def cc(C):
    from lte_phy import channel_coding
    return channel_coding


def typed(llr, prec):
    out = llr.astype(np.float32 if prec == 'f32' else np.float64)
    assert np.array_equal(out.astype(np.float64), llr)                 # the grid values are float32 values
    return out


def differing(bits, want):
    return np.flatnonzero((bits != want).any(axis=1)).tolist()


def check_known_lanes(p, ln, bits, n, what):
    """The known-answer lanes against their construction (n: the iterations, one
    number or one per lane); returns how many lanes had a known answer."""
    seen = 0
    for lane in np.flatnonzero(p.kind[ln] != 0):
        want = X.known_answer(p, ln[lane], n[lane] if np.ndim(n) else n)
        if want is not None:
            assert np.array_equal(bits[lane], want), (what, int(lane), int(p.kind[ln[lane]]))
            seen += 1
    return seen


# ---------------------------------------------------------------------------
# (1)
@pytest.mark.parametrize('K', X.KS)
def test_pool_conditions(oracle, K):
    X.assert_pool_conditions(oracle, K)


# ---------------------------------------------------------------------------
# (2)
@pytest.mark.parametrize('K,quant,prec', CASES)
def test_fixed_decoder_equals_the_reference(cc, oracle, K, quant, prec):
    p, D, ln = X.quant_pool(oracle, K, quant), X.reference(oracle, K, quant), X.lanes(oracle, K, quant)
    llr = typed(p.llr, prec)[ln]
    for iters in (0, 1, 2, ITERS):
        bits = cc.turbo_decode_batch(llr, K, iters, prec)
        want = D[ln, iters]            # iters 1, 2, 8: oracle.turbo_decode itself (exact_llr_model.reference)
        assert np.array_equal(bits, want), (K, quant, prec, iters, differing(bits, want))
        assert check_known_lanes(p, ln, bits, iters, (K, quant, prec, iters)) >= 5 * 6
        assert np.array_equal(bits[65:128:2], want[65:128:2])          # the known-answer lanes' neighbours


# ---------------------------------------------------------------------------
# (3)
@pytest.mark.parametrize('K,quant,prec', CASES)
def test_early_stop_follows_the_rule_on_the_reference(cc, oracle, K, quant, prec):
    p, D, ln = X.quant_pool(oracle, K, quant), X.reference(oracle, K, quant), X.lanes(oracle, K, quant)
    llr = typed(p.llr, prec)[ln]
    for crc in POLYS:
        n_star, passed = X.rules(oracle, D, crc)
        want_n = n_star[ln]
        want = D[ln, want_n]
        assert len(set(want_n[:64][passed[ln][:64]].tolist())) >= 2 and not passed[ln][:64].all()
        for repack in (None, 1, 3):
            res = cc.turbo_decode_early_stop(llr, K, ITERS, crc, precision=prec, repack=repack)
            bits, used = res[0], res[1]
            what = (K, quant, prec, crc, repack)
            assert np.array_equal(used, want_n), (what, used.tolist(), want_n.tolist())
            assert np.array_equal(bits, want), (what, differing(bits, want))
            assert check_known_lanes(p, ln, bits, used, what) >= 5 * 6
            for lane in np.flatnonzero(p.kind[ln] != 0):
                k = X.known_n_star(p, ln[lane], crc)
                assert k is None or used[lane] == k, (what, int(lane))
            assert np.array_equal(bits[65:128:2], want[65:128:2]) and np.array_equal(used[65:128:2], want_n[65:128:2])
            if repack:
                und = int(np.sum([all(oracle.crc_bits(D[b, n], POLYS[crc], 24).any() for n in range(1, repack + 1))
                                  for b in ln]))
                assert res[2]['undecided'] == und and und > 0, (what, res[2], und)


# ---------------------------------------------------------------------------
# (4)
@pytest.mark.parametrize('K,quant,prec', CASES)
def test_scaled_decoders_equal_the_reference(C, oracle, K, quant, prec):
    p, D, ln = X.quant_pool(oracle, K, quant), X.reference_scaled(oracle, K, quant), X.lanes(oracle, K, quant)
    D1 = X.reference(oracle, K, quant)
    llr = typed(p.llr, prec)[ln]
    for iters in (1, SC_ITERS):
        bits = C.turbo_decode_scaled(llr, K, iters, SC_SCALE, prec)
        assert np.array_equal(bits, D[ln, iters]), (K, quant, prec, iters, differing(bits, D[ln, iters]))
        assert check_known_lanes(p, ln, bits, iters, (K, quant, prec, iters)) >= 5 * 6
    assert (D[:, SC_ITERS] != D1[:, SC_ITERS]).any()                   # the scale shows in the reference's decisions
    for crc in POLYS:
        n_star, _ = X.rules(oracle, D, crc)
        want_n, want = n_star[ln], D[ln, n_star[ln]]
        for after in (0, 1):
            bits, used, _ = C.turbo_decode_es_scaled(llr, K, SC_ITERS, POLYS[crc], SC_SCALE, after, prec)
            what = (K, quant, prec, crc, after)
            assert np.array_equal(used, want_n), (what, used.tolist(), want_n.tolist())
            assert np.array_equal(bits, want), (what, differing(bits, want))
            assert check_known_lanes(p, ln, bits, used, what) >= 5 * 6


# ---------------------------------------------------------------------------
# (5)
@pytest.mark.parametrize('quant', list(X.QUANT))
@pytest.mark.parametrize('K', [40, 1056])
def test_bcjr_values_equal_the_oracle(C, oracle, K, quant):
    """One wave and a partial one.  ls, lp of a pool block; la the extrinsic of
    the reference's first iteration (on the grid, and not trivial)."""
    p = X.quant_pool(oracle, K, quant)
    idx = np.arange(64 + 3) % len(p.llr)
    ls = np.array([np.concatenate([l[0:3 * K:3], l[3 * K:3 * K + 3]]) for l in p.llr])
    lp = np.array([np.concatenate([l[1:3 * K:3], l[3 * K + 3:3 * K + 6]]) for l in p.llr])
    la = np.array([np.concatenate([oracle.turbo_decode(l, K, 1, trace=True)[1][0], np.zeros(3)]) for l in p.llr])
    ref = np.array([oracle.bcjr_app(a, b, c) for a, b, c in zip(ls, lp, la)])
    assert np.isfinite(ref).all()                                      # no position to leave out of the f32 comparison
    assert (la != 0).any() and (ref[p.kind != X.ZERO][:, :K] == 0).sum() >= 8      # ties among the values, beside the all-zero block's
    ls, lp, la, ref = ls[idx], lp[idx], la[idx], ref[idx]
    app = np.zeros_like(ref)
    C.check(C.load().lte_bcjr_host64(K + 3, len(idx), *[C.ptr(np.ascontiguousarray(v), C.F64) for v in (ls, lp, la)],
                                     C.ptr(app, C.F64)))
    assert np.array_equal(app, ref), (K, quant, 'f64', int(np.sum(app != ref)))
    f = [typed(v, 'f32') for v in (ls, lp, la)]
    app32 = np.full((len(idx), K), np.nan, dtype=np.float32)
    C.check(C.load().lte_bcjr_host(K, len(idx), *[C.ptr(np.ascontiguousarray(v), C.F32) for v in f],
                                   C.ptr(app32, C.F32)))
    bad = np.argwhere(app32.astype(np.float64) != ref[:, :K])
    assert np.array_equal(app32.astype(np.float64), ref[:, :K]), (K, quant, 'f32', len(bad), bad[:4].tolist())


# ---------------------------------------------------------------------------
# (6)
_GAUSS = {}


def gauss(O, K):
    if K not in _GAUSS:
        _GAUSS[K] = X.gaussian_blocks(O, K, 64 + 3)
    return _GAUSS[K]


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('K', [40, 1056, 6144])
def test_decoders_are_scale_invariant(cc, oracle, K, prec):
    llr, sent = gauss(oracle, K)
    base = llr.astype(np.float32 if prec == 'f32' else np.float64)
    bits = cc.turbo_decode_batch(base, K, ITERS, prec)
    ok = (bits == sent).all(axis=1)
    assert ok.sum() >= 16 and (~ok).sum() >= 16, (K, prec, int(ok.sum()))          # both sides of the cliff
    es_bits, es_used = cc.turbo_decode_early_stop(base, K, ITERS, '24B', precision=prec)
    assert len(set(es_used.tolist())) >= 3
    for k in ((200, -200) if prec == 'f64' else (64, -64)):
        scaled = base * base.dtype.type(2.0 ** k)
        assert np.array_equal(scaled.astype(np.float64), llr * 2.0 ** k)           # exact, and normal numbers
        assert np.isfinite(scaled).all() and (np.abs(scaled[scaled != 0]) > np.finfo(base.dtype).tiny * 2.0 ** 30).all()
        b = cc.turbo_decode_batch(scaled, K, ITERS, prec)
        assert np.array_equal(b, bits), (K, prec, k, differing(b, bits))
        b, u = cc.turbo_decode_early_stop(scaled, K, ITERS, '24B', precision=prec)
        assert np.array_equal(u, es_used) and np.array_equal(b, es_bits), (K, prec, k, differing(b, es_bits))
