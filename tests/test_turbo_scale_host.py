"""CPU: extrinsic scaling of the turbo decoders (scaled max-log-MAP) -- the C
ABI additions (header, exports, ctypes signatures, refusals that return before
the device is touched), the models of tests/turbo_scaled_model.py against the
oracle, the benefit the feature is built for, the Python surface, and the
conditions on the pools of the GPU stage tests.  The kernels are held to the
models, exactly, in tests/test_gpu_turbo_scale.py."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import turbo_scaled_model as M
from conftest import ROOT

NEW_SYMBOLS = {'lte_plan_set_turbo_scale': 'int', 'lte_plan_turbo_scale': 'double',
               'lte_turbo_decode_scaled_host64': 'int', 'lte_turbo_decode_scaled_host': 'int',
               'lte_turbo_decode_es_scaled_host64': 'int', 'lte_turbo_decode_es_scaled_host': 'int'}
CRC24B = 0x1800063
BAD_SCALES = (0.0, -0.5, 1.0000001, float('nan'), float('inf'))


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


# ---------------------------------------------------------------------------
# interface
def test_header_declares_the_six_prototypes():
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    for name, res in NEW_SYMBOLS.items():
        assert re.search(r'^%s %s\(' % (res, name), text, re.M), name
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)       # additions only


def test_header_and_model_state_the_definition_in_the_same_words():
    """The definition's sentences, with the comment frames and line breaks taken out."""
    def words(s):
        return ' '.join(re.sub(r'^\s*\*', '', ln).strip() for ln in s.splitlines()).split()

    head = ' '.join(words(open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()))
    model = ' '.join(words(M.__doc__))
    start, end = 'A scale s is a number', 'bit for bit the unscaled one.'
    a = head[head.index(start):head.index(end) + len(end)]
    b = model[model.index(start):model.index(end) + len(end)]
    assert a == b and 'e = s * ((L - La) - Ls)' in a


def test_library_exports_them_with_signatures(C):
    lib = C.load()
    for name in NEW_SYMBOLS:
        assert name in C._SIGS, name
        assert getattr(lib, name).argtypes == C._SIGS[name][1], name
        assert getattr(lib, name).restype == C._SIGS[name][0], name
    assert C._SIGS['lte_plan_turbo_scale'][0] is C.c_f64
    assert lib.lte_version() == 3


# ---------------------------------------------------------------------------
# refusals before the device is touched (no GPU here: a HIP call would fail otherwise)
def test_plan_entries_refuse_a_null_plan(C):
    lib = C.load()
    for s in (0.75, 1.0) + BAD_SCALES:
        assert lib.lte_plan_set_turbo_scale(None, s) == C.LTE_EINVAL
    assert math.isnan(lib.lte_plan_turbo_scale(None))


@pytest.mark.parametrize('f64', [True, False])
def test_stage_entries_refuse_bad_arguments_without_a_device(C, f64):
    dt, ct = (np.float64, C.F64) if f64 else (np.float32, C.F32)
    lib = C.load()
    fx = lib.lte_turbo_decode_scaled_host64 if f64 else lib.lte_turbo_decode_scaled_host
    es = lib.lte_turbo_decode_es_scaled_host64 if f64 else lib.lte_turbo_decode_es_scaled_host
    llr, bits, used = np.ones((2, 132), dtype=dt), np.zeros((2, 40), dtype=np.uint8), np.zeros(2, dtype=np.uint8)
    info = np.zeros(3, dtype=np.int64)

    def fixed(K=40, iters=8, scale=0.75):
        return fx(K, iters, 2, C.ptr(llr, ct), scale, C.ptr(bits, C.U8))

    def stop(K=40, iters=8, poly=CRC24B, scale=0.75, after=0, null=None):
        a = {'llr': C.ptr(llr, ct), 'bits': C.ptr(bits, C.U8), 'used': C.ptr(used, C.U8), 'info': C.ptr(info, C.c_i64)}
        if null:
            a[null] = None
        return es(K, iters, 2, a['llr'], poly, scale, after, a['bits'], a['used'], a['info'])

    for s in BAD_SCALES:
        assert fixed(scale=s) == C.LTE_EINVAL, s
        assert b'scale' in lib.lte_last_error()
        assert stop(scale=s) == C.LTE_EINVAL, s
        assert stop(scale=s, after=1) == C.LTE_EINVAL, s
    assert fixed(K=41) == C.LTE_EINVAL and b'K=41' in lib.lte_last_error()       # outside the 188 sizes
    assert fixed(K=41, scale=1.0) == C.LTE_EINVAL
    assert fixed(iters=-1) == C.LTE_EINVAL
    assert stop(K=41) == C.LTE_EINVAL and b'K=41' in lib.lte_last_error()
    assert stop(iters=-1) == C.LTE_EINVAL
    assert stop(poly=0x11021) == C.LTE_EINVAL
    for null in ('llr', 'bits', 'used'):
        assert stop(null=null) == C.LTE_EINVAL, null
    assert stop(after=1, null='info') == C.LTE_EINVAL                            # info only with a boundary
    for iters, after in ((8, 8), (8, -1), (8, 9), (1, 1)):
        assert stop(iters=iters, after=after) == C.LTE_EINVAL, (iters, after)
        assert b'boundary' in lib.lte_last_error()


# ---------------------------------------------------------------------------
# the models against the oracle
def noisy_block(O, K, snr, rs):
    cb = rs.randint(0, 2, K).astype(np.uint8)
    s2 = 10 ** (-snr / 10)
    return cb, 2 * (1 - 2.0 * O.turbo_encode(cb) + np.sqrt(s2) * rs.randn(3 * K + 12)) / s2


@pytest.mark.parametrize('K', [40, 56, 1056, 6144])
def test_models_at_scale_one_are_the_oracle(oracle, K):
    rs = np.random.RandomState(K)
    for snr in (2.0, 3.0):
        _, llr = noisy_block(oracle, K, snr, rs)
        l32 = llr.astype(np.float32)
        D, D32 = M.decisions(oracle, llr, K, 8), M.decisions(oracle, l32, K, 8, f32=True)
        for it in (0, 1, 2, 8):
            ref = oracle.turbo_decode(llr, K, it)
            assert np.array_equal(M.turbo_decode_scaled(oracle, llr, K, it, 1.0), ref), (K, it)
            assert np.array_equal(D[it], ref), (K, it)                 # one pass gives every D(n)
            ref = oracle.turbo_decode_f32_model(l32, K, it)
            assert np.array_equal(M.turbo_decode_scaled(oracle, l32, K, it, 1.0, True), ref), (K, it)
            assert np.array_equal(D32[it], ref), (K, it)


def test_scaling_decodes_more_blocks(oracle):
    """What the feature is for: K = 6144 at 3.0 dB, 40 blocks, 8 iterations."""
    K = 6144
    rs = np.random.RandomState(7 * 6144 + 300)
    errs = {1.0: 0, 0.75: 0}
    for _ in range(40):
        cb, llr = noisy_block(oracle, K, 3.0, rs)
        for s in errs:
            errs[s] += int(np.any(M.turbo_decode_scaled(oracle, llr, K, 8, s) != cb))
    print(f'block errors of 40: scale 1 {errs[1.0]}, scale 0.75 {errs[0.75]}')
    assert errs[0.75] < errs[1.0], errs


# ---------------------------------------------------------------------------
# Python surface
def test_python_surface():
    import lte_phy
    from lte_phy import channel_coding, engine, ofdm_core
    params = inspect.signature(engine.Plan.__init__).parameters
    p = params['turbo_scale']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None and list(params)[-1] == 'turbo_scale'
    assert isinstance(engine.Plan.turbo_scale, property) and callable(engine.Plan.set_turbo_scale)
    assert lte_phy.OFDMSimulator.turbo_scale == 1.0
    assert 'turbo_scale' not in inspect.signature(lte_phy.OFDMSimulator.__init__).parameters
    assert len(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters) == 17
    assert inspect.signature(ofdm_core._spatial_plan).parameters['turbo_scale'].default is None
    assert len(channel_coding.__all__) == 18 and 'turbo_decode_scaled' not in channel_coding.__all__
    sig = inspect.signature(channel_coding.turbo_decode_scaled)
    assert [(p.name, p.default) for p in sig.parameters.values()] == \
        [('llr', inspect.Parameter.empty), ('K', inspect.Parameter.empty), ('num_iterations', 8), ('scale', 0.75)]
    assert 'scale' not in inspect.signature(channel_coding.turbo_decode).parameters
    assert 'scale' not in inspect.signature(channel_coding.turbo_decode_early_stop).parameters
    assert 'turbo_scale' not in inspect.signature(lte_phy.simulate_spatial_multiplexing_coded).parameters


def test_plan_cache_key_holds_the_scale(C):
    from lte_phy import engine
    kw = dict(N=128, Nc=72, cp_len=9, bps=2, n_sym=0, chain=C.CHAIN_CODED, channel=C.CH_AWGN, fs=1.92e6, n_bits=40,
              max_frames=4)
    plain, off, one = (engine.plan_key(**kw, **x)[0] for x in ({}, {'turbo_scale': None}, {'turbo_scale': 1}))
    assert plain == off == one
    a, b = engine.plan_key(**kw, turbo_scale=0.75)[0], engine.plan_key(**kw, turbo_scale=0.5)[0]
    assert a != plain and b != plain and a != b
    assert set(a) - set(plain) == {('turbo_scale', 0.75)}


def test_python_refusals_come_before_the_device(monkeypatch):
    from lte_phy import _capi, channel_coding, engine

    def trap(*a, **k):
        raise AssertionError('the device was touched')

    monkeypatch.setattr(_capi, 'device_init', trap)
    monkeypatch.setattr(_capi, 'load', trap)
    kw = dict(N=128, Nc=72, cp_len=9, bps=2, n_sym=0, chain=_capi.CHAIN_CODED, channel=_capi.CH_AWGN, fs=1.92e6,
              n_bits=40, max_frames=4)
    for bad in BAD_SCALES:
        with pytest.raises(ValueError, match='turbo_scale'):
            engine.Plan(**kw, turbo_scale=bad)
        with pytest.raises(ValueError, match='turbo_scale'):
            engine.get_plan(**kw, turbo_scale=bad)
        with pytest.raises(ValueError, match='turbo_scale'):
            channel_coding.turbo_decode_scaled(np.zeros(132), 40, 8, bad)


# ---------------------------------------------------------------------------
# the pools of the GPU stage tests: a kernel that ignored the scale must not pass
POOLS = [(K, crc, f32, s) for K in sorted(M.STAGE) for crc in ('24A', '24B') for f32 in (False, True)
         for s in sorted(set(M.SCALES[f32]) | {M.ES_SCALE})]


@pytest.mark.parametrize('K,crc,f32,scale', POOLS)
def test_stage_pool_conditions(oracle, K, crc, f32, scale):
    differ, n_star_differ, mixes = M.pool_conditions(oracle, K, crc, f32, scale)
    assert differ >= 3, (K, crc, f32, scale, differ)               # scaled D(8) != unscaled D(8)
    assert n_star_differ >= 3, (K, crc, f32, scale, n_star_differ)   # n* differs under the rule
    assert mixes, (K, crc, f32, scale)                             # `mixing` on the scaled n*
    _, D, n_star, passed = M.stage_pool(oracle, K, crc, f32, scale)
    assert passed[-1] and n_star[-1] == 1 and not D[-1].any()      # the all-zero word
    # the fixed-decoder tests' other iteration counts tell the scale too
    _, D1, _, _ = M.stage_pool(oracle, K, crc, f32, 1.0)
    for it in (1, 2):
        assert (D[:, it] != D1[:, it]).any(), (K, crc, f32, scale, it)
