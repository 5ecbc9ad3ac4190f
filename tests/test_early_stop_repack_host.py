"""CPU: the interface of re-packing the early-stop decoders' undecided blocks --
the C ABI additions (header, exports, ctypes signatures, refusals that return
before the device is touched) and the Python keywords.  The kernels are checked
on the GPU in tests/test_gpu_early_stop_repack.py."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ['lte_plan_set_early_stop_repack', 'lte_plan_early_stop_repack', 'lte_plan_repack_info',
               'lte_turbo_decode_es_repack_host64', 'lte_turbo_decode_es_repack_host']
CRC24B = 0x1800063


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def sim():
    import lte_phy
    return lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % name, text, re.M), name
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)       # additions only


def test_library_exports_them_with_signatures(C):
    lib = C.load()
    for name in NEW_SYMBOLS:
        assert name in C._SIGS, name
        assert getattr(lib, name).argtypes == C._SIGS[name][1], name
    assert lib.lte_version() == 3


def test_plan_entries_refuse_a_null_plan(C):
    lib = C.load()
    assert lib.lte_plan_set_early_stop_repack(None, 1) == C.LTE_EINVAL
    assert lib.lte_plan_set_early_stop_repack(None, 0) == C.LTE_EINVAL
    assert lib.lte_plan_early_stop_repack(None) == C.LTE_EINVAL
    info = np.zeros(8, dtype=np.int64)
    assert lib.lte_plan_repack_info(None, C.ptr(info, C.c_i64), 8) == C.LTE_EINVAL


@pytest.mark.parametrize('f64', [True, False])
def test_stage_entries_refuse_bad_arguments_without_a_device(C, f64):
    """The early-stop entries' refusals, then the boundary outside 1..iters-1 and
    a NULL info: LTE_EINVAL and no HIP call before it (no GPU is needed here)."""
    dt, ct = (np.float64, C.F64) if f64 else (np.float32, C.F32)
    f = C.load().lte_turbo_decode_es_repack_host64 if f64 else C.load().lte_turbo_decode_es_repack_host
    llr, bits, used = np.ones((2, 132), dtype=dt), np.zeros((2, 40), dtype=np.uint8), np.zeros(2, dtype=np.uint8)
    info = np.zeros(3, dtype=np.int64)

    def call(K=40, iters=8, poly=CRC24B, after=1, null=None):
        a = {'llr': C.ptr(llr, ct), 'bits': C.ptr(bits, C.U8), 'used': C.ptr(used, C.U8), 'info': C.ptr(info, C.c_i64)}
        if null:
            a[null] = None
        return f(K, iters, 2, a['llr'], poly, after, a['bits'], a['used'], a['info'])

    assert call(K=41) == C.LTE_EINVAL and b'K=41' in C.load().lte_last_error()
    assert call(iters=-1) == C.LTE_EINVAL
    assert call(poly=0x11021) == C.LTE_EINVAL
    for null in ('llr', 'bits', 'used', 'info'):
        assert call(null=null) == C.LTE_EINVAL, null
    for iters, after in ((8, 0), (8, 8), (8, -1), (8, 9), (1, 1), (0, 0)):
        assert call(iters=iters, after=after) == C.LTE_EINVAL, (iters, after)
        assert b'boundary' in C.load().lte_last_error()


def test_keywords_are_carried():
    from lte_phy import channel_coding, engine, ofdm_core
    p = inspect.signature(engine.Plan.__init__).parameters['repack']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    p = inspect.signature(channel_coding.turbo_decode_early_stop).parameters['repack']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for f in (ofdm_core.OFDMSimulator._plan, ofdm_core.OFDMSimulator._sfbc_plan, ofdm_core._spatial_plan):
        assert inspect.signature(f).parameters['repack'].default is None, f


def test_boundary_rule():
    """What a repack= keyword stands for: off, the default boundary, or its own."""
    from lte_phy.engine import REPACK_DEFAULT, repack_boundary
    assert REPACK_DEFAULT == 1
    for off in (None, False, 0):
        assert repack_boundary(off, True, 8) == 0 and repack_boundary(off, False, 8) == 0
    assert repack_boundary(True, True, 8) == REPACK_DEFAULT
    assert [repack_boundary(a, True, 8) for a in (1, 2, 7)] == [1, 2, 7]
    assert repack_boundary(1, True, 2) == 1
    for after, es, iters in ((1, False, 8), (True, False, 8), (8, True, 8), (-1, True, 8), (9, True, 8), (1, True, 1),
                             (True, True, 1), (1, True, 0)):
        with pytest.raises(ValueError, match='repack'):
            repack_boundary(after, es, iters)


def test_python_refusals_come_before_the_device(monkeypatch):
    """repack without early_stop, or a boundary outside 1..turbo_iters-1:
    ValueError from Plan, get_plan, both grid drivers and the stage entry, with
    the device initialisation replaced by a trap."""
    from lte_phy import _capi, channel_coding, engine

    def trap(*a, **k):
        raise AssertionError('the device was touched')

    monkeypatch.setattr(_capi, 'device_init', trap)
    monkeypatch.setattr(_capi, 'load', trap)
    kw = dict(N=128, Nc=72, cp_len=9, bps=2, n_sym=0, chain=_capi.CHAIN_CODED, channel=_capi.CH_AWGN, fs=1.92e6,
              n_bits=40, max_frames=4)
    s = sim()
    for bad in (dict(repack=1), dict(repack=True), dict(early_stop=True, repack=8), dict(early_stop=True, repack=-1),
                dict(early_stop=True, turbo_iters=1, repack=True)):
        with pytest.raises(ValueError, match='repack'):
            engine.Plan(**kw, **bad)
        with pytest.raises(ValueError, match='repack'):
            engine.get_plan(**kw, **bad)
        with pytest.raises(ValueError, match='repack'):
            s.run_grid([0.0], 1, coded=True, **bad)
        with pytest.raises(ValueError, match='repack'):
            s.run_grid([0.0], 1, coded=True, mimo='sfbc', num_rx=2, **bad)
        with pytest.raises(ValueError, match='repack'):
            s.run_scfdm_grid([0.0], 1, **bad)
    assert s._repack == 0                                              # nothing left behind by a refused call
    for after in (8, -2):
        with pytest.raises(ValueError, match='repack'):
            channel_coding.turbo_decode_early_stop(np.zeros(132), 40, 8, repack=after)
    with pytest.raises(ValueError, match='repack'):
        channel_coding.turbo_decode_early_stop(np.zeros(132), 40, 1, repack=True)


def test_grid_drivers_keep_their_parameter_lists():
    """`repack` is one more keyword of run_grid / run_scfdm_grid; the parameters
    the other host tests pin stay as they are."""
    import lte_phy
    assert list(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters)[-1] == 'early_stop'
    assert list(inspect.signature(lte_phy.OFDMSimulator.run_scfdm_grid).parameters)[-1] == 'early_stop'
    assert 'repack' in lte_phy.OFDMSimulator.run_grid.__doc__
