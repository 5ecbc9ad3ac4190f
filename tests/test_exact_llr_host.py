"""CPU: the exact tie between the float32 decoder models and the reference.

On the pools of tests/exact_llr_model.py (LLRs on a power-of-two grid) every
value of max-log-MAP is exactly representable in float32, so the float32 models
-- oracle.turbo_decode_f32_model, which the k_turbo tests compare the kernels
with, and tests/turbo_scaled_model.c -- must give oracle.turbo_decode's
decisions on every block and after every iteration, below the cliff as well as
above it.  tests/test_turbo_model.py ties them on converging blocks and
statistically; this is the exact tie, and tests/test_gpu_exact_llr.py holds the
kernels themselves to the same reference.

  (1) the premise: exactness_audit on every pool block
  (2) the f32 models equal the reference, D(1) .. D(iters), scale 1 and 0.5
  (3) the known-answer blocks decode to what their construction says
  (4) the pools' conditions (a wrong kernel could not pass)
  (5) the models are invariant under a power-of-two scale of the LLRs, and
      where the float32 model (-1e30 sentinels) stops being so
"""
import numpy as np
import pytest

import exact_llr_model as X
import turbo_scaled_model as M

ITERS, SC_ITERS, SC_SCALE = X.ITERS, X.SC_ITERS, X.SC_SCALE


# ---------------------------------------------------------------------------
# (1)
@pytest.mark.parametrize('K', X.KS)
def test_premise_every_value_is_on_the_grid(oracle, K):
    pools = [X.quant_pool(oracle, K, quant) for quant in X.QUANT]
    llr = np.concatenate([p.llr for p in pools])
    step = np.concatenate([np.full(len(p.llr), X.QUANT[quant][0]) for p, quant in zip(pools, X.QUANT)])
    worst = 0.0
    for iters, scale, ref in ((ITERS, 1.0, X.reference), (SC_ITERS, SC_SCALE, X.reference_scaled)):
        a = X.exactness_audit(oracle, llr, K, iters, scale, step=step)             # the three grids in one evaluation
        assert np.array_equal(a.q, step / 2 / (1 if scale == 1.0 else 2 ** (2 * iters)))
        assert a.exact, (K, scale)
        assert a.ratio < X.RATIO_BOUND, (K, scale, a.ratio)
        # the audit is an evaluation of its own; it decides what the oracle decides
        assert np.array_equal(a.D, np.concatenate([ref(oracle, K, quant) for quant in X.QUANT])), (K, scale)
        worst = max(worst, a.ratio)
    print(f'K={K}: worst |value| / q = {worst:.0f} = 2^{np.log2(worst):.2f} (bound 2^22)')


def test_audit_notices_an_inexact_scale_and_finds_the_step(oracle):
    p = X.quant_pool(oracle, 40, 's025')
    assert X.exactness_audit(oracle, p.llr[:4], 40, 2).q == 0.125                  # the step, from the data
    off = p.llr[:4].copy()
    off[0, 5] += 2.0 ** -20
    assert not X.exactness_audit(oracle, off, 40, 2, step=0.25).exact


# ---------------------------------------------------------------------------
# (2)
@pytest.mark.parametrize('K', X.KS)
def test_f32_models_equal_the_reference(oracle, K):
    O = oracle
    for quant in X.QUANT:
        p = X.quant_pool(O, K, quant)
        D, Ds = X.reference(O, K, quant), X.reference_scaled(O, K, quant)
        for b, llr in enumerate(p.llr):
            l32 = llr.astype(np.float32)
            assert np.array_equal(l32.astype(np.float64), llr)
            for n in range(1, ITERS + 1):
                want = O.turbo_decode(llr, K, n)
                assert np.array_equal(D[b, n], want), (K, quant, b, n)             # the restated loop is the oracle's
                assert np.array_equal(O.turbo_decode_f32_model(l32, K, n), want), (K, quant, b, n)
            assert np.array_equal(M.decisions_f32(O, l32, K, ITERS), D[b]), (K, quant, b)
            assert np.array_equal(M.decisions_f32(O, l32, K, SC_ITERS, SC_SCALE), Ds[b]), (K, quant, b)


# ---------------------------------------------------------------------------
# (3)
@pytest.mark.parametrize('K', X.KS)
def test_known_answers(oracle, K):
    for quant in X.QUANT:
        p = X.quant_pool(oracle, K, quant)
        assert sorted(p.kind[p.kind != 0].tolist()) == [1, 2, 3, 4, 5, 6]
        for D in (X.reference(oracle, K, quant), X.reference_scaled(oracle, K, quant)):
            seen = 0
            for b in np.flatnonzero(p.kind != 0):
                for n in range(D.shape[1]):
                    want = X.known_answer(p, b, n)
                    if want is not None:
                        assert np.array_equal(D[b, n], want), (K, quant, int(p.kind[b]), n)
                        seen += 1
                for crc in X.POLYS:
                    n_star = X.rules(oracle, D[b:b + 1], crc)[0][0]
                    want = X.known_n_star(p, b, crc)
                    assert want is None or n_star == want, (K, quant, int(p.kind[b]), crc)
            assert seen == 5 * D.shape[1] + 1
        # the parity-free block is not a trivial one: its decisions are not the systematic signs
        b = int(np.flatnonzero(p.kind == X.NOPAR)[0])
        assert not np.array_equal(X.known_answer(p, b, 0), p.llr[b][0:3 * K:3] < 0)


# ---------------------------------------------------------------------------
# (4)
@pytest.mark.parametrize('K', X.KS)
def test_pool_conditions(oracle, K):
    c = X.assert_pool_conditions(oracle, K)
    tz = X.ties(oracle, K)
    print(f"K={K}: {c['ties']} exact ties L == 0 after {ITERS} iterations in {len(tz)} step-1.0 blocks, "
          f"{c['ties_that_matter']} of them in an otherwise decoded block or at a sent 1; "
          f"decoded {c['decoded']}, wave-0 n* {c['n_star']}")
    for quant in X.QUANT:
        p = X.quant_pool(oracle, K, quant)
        ln = X.lanes(oracle, K, quant)
        assert len(ln) == X.NCB and len(p.kind) <= 64 and set(ln[:64].tolist()) == set(range(len(p.kind)))
        ok = (X.reference(oracle, K, quant)[:, ITERS] == p.sent).all(axis=1)
        # wave 1: a known-answer lane's neighbours are ladder blocks the reference fails
        assert (p.kind[ln[64:128:2]] != 0).all() and (p.kind[ln[65:128:2]] == 0).all() and not ok[ln[65:128:2]].any()
        assert set(p.kind[ln[64:128:2]].tolist()) == {1, 2, 3, 4, 5, 6}
        assert len({tuple(l) for l in p.llr}) == len(p.llr)                        # distinct blocks
        if X.QUANT[quant][2]:
            z = np.mean(p.llr[p.kind == 0] == 0.0)
            assert 0.2 < z < 0.5, z                                                # erasures, by the thousand
        assert not np.signbit(p.llr[p.llr == 0]).any()


# ---------------------------------------------------------------------------
# (5)
def scale_blocks(O, K):
    """One block the reference decodes and one it fails, unquantised."""
    llr, sent = X.gaussian_blocks(O, K, 12)
    ok = np.array([np.array_equal(O.turbo_decode(l, K, ITERS), s) for l, s in zip(llr, sent)])
    assert ok.any() and not ok.all()
    return llr[[np.flatnonzero(ok)[0], np.flatnonzero(~ok)[-1]]]


@pytest.mark.parametrize('K', X.KS)
def test_models_are_scale_invariant(oracle, K):
    for llr in scale_blocks(oracle, K):
        l32 = llr.astype(np.float32)
        d64, d32 = M.decisions_f64(oracle, llr, K, ITERS), M.decisions_f32(oracle, l32, K, ITERS)
        for k in (200, -200):
            assert np.array_equal(M.decisions_f64(oracle, llr * 2.0 ** k, K, ITERS), d64), (K, k)
        for k in (64, -64):
            scaled = l32 * np.float32(2.0 ** k)
            assert np.array_equal(scaled.astype(np.float64), llr * 2.0 ** k)       # normal numbers, exact
            assert np.array_equal(M.decisions_f32(oracle, scaled, K, ITERS), d32), (K, k)


def first_change(O, l32, K, ks):
    base = M.decisions_f32(O, l32, K, ITERS)[ITERS]
    for k in ks:
        with np.errstate(over='ignore'):
            scaled = l32 * np.float32(2.0) ** np.float32(k)
        if not np.isfinite(scaled).all():
            break
        if not np.array_equal(M.decisions_f32(O, scaled, K, ITERS)[ITERS], base):
            return k
    return None


def test_where_the_f32_model_stops_being_invariant(oracle):
    """The float32 decoders start their metrics at -1e30 (LTE_NEG_BIG), about
    -2^99.7: once sums of LLRs come near it, an unreachable state wins a max.
    Upward the first exponent at which a decision of D(8) changes is printed (it
    is what include/lte_phy.h and DESIGN.md section 5 state) and only asserted
    to be at least 64; downward float32 runs out of normal numbers first."""
    up, down = [], []
    for K in X.KS:
        for llr in scale_blocks(oracle, K):
            l32 = llr.astype(np.float32)
            up.append(first_change(oracle, l32, K, range(64, 128, 4)))
            down.append(first_change(oracle, l32, K, range(-64, -152, -4)))
            print(f'K={K}: max |LLR| = {np.abs(l32).max():.1f}, D(8) first changes at 2^{up[-1]} and 2^{down[-1]}')
    first_up = min(k for k in up if k is not None)
    print(f'the float32 model: D(8) is unchanged by 2^k for {max(k for k in down if k is not None) + 4} <= k <= '
          f'{first_up - 4} on every block; the first change upward is at k = {first_up}')
    assert first_up >= 64 and all(k is None or k <= -64 for k in down)
