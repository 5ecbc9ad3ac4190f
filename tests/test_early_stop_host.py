"""CPU: the interface of the turbo decoders' CRC early termination -- the C ABI
additions (header, exports, ctypes signatures, argument checks that return
before the device is touched) and the Python keywords.  The kernels themselves
are checked on the GPU in tests/test_gpu_early_stop.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ['lte_plan_set_early_stop', 'lte_plan_early_stop', 'lte_plan_turbo_iters_used',
               'lte_turbo_decode_es_host64', 'lte_turbo_decode_es_host']
CRC24A, CRC24B = 0x1864CFB, 0x1800063


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % name, text, re.M), name
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)


def test_library_exports_them_with_signatures(C):
    lib = C.load()
    for name in NEW_SYMBOLS:
        assert name in C._SIGS, name
        assert getattr(lib, name).argtypes == C._SIGS[name][1], name
    assert lib.lte_version() == 3 and C.ABI_VERSION == 3


def _es_call(C, f64, K, iters, poly, ncb=2, null=None):
    dt, ct = (np.float64, C.F64) if f64 else (np.float32, C.F32)
    n = 3 * max(K, 0) + 12
    llr = np.ones((ncb, n), dtype=dt)
    bits = np.zeros((ncb, max(K, 1)), dtype=np.uint8)
    used = np.zeros(ncb, dtype=np.uint8)
    a = {'llr': C.ptr(llr, ct), 'bits': C.ptr(bits, C.U8), 'used': C.ptr(used, C.U8)}
    if null:
        a[null] = None
    f = C.load().lte_turbo_decode_es_host64 if f64 else C.load().lte_turbo_decode_es_host
    return f(K, iters, ncb, a['llr'], poly, a['bits'], a['used'])


@pytest.mark.parametrize('f64', [True, False])
def test_stage_entries_refuse_bad_arguments_without_a_device(C, f64):
    """K outside the 188 sizes, negative iters, a generator that is not one of
    the two CRC-24s, NULL pointers: LTE_EINVAL, and no HIP call before it (this
    test runs where there is no GPU)."""
    assert _es_call(C, f64, 41, 8, CRC24B) == C.LTE_EINVAL
    assert b'K=41' in C.load().lte_last_error()
    assert _es_call(C, f64, 40, -1, CRC24B) == C.LTE_EINVAL
    assert _es_call(C, f64, 40, 8, 0x11021) == C.LTE_EINVAL
    assert b'crc_poly' in C.load().lte_last_error()
    assert _es_call(C, f64, 40, 8, CRC24A & 0xFFFFFF) == C.LTE_EINVAL      # without its x^24 term
    for null in ('llr', 'bits', 'used'):
        assert _es_call(C, f64, 40, 8, CRC24A, null=null) == C.LTE_EINVAL, null


def test_plan_entries_refuse_a_null_plan(C):
    lib = C.load()
    assert lib.lte_plan_set_early_stop(None, 1) == C.LTE_EINVAL
    assert lib.lte_plan_early_stop(None) == C.LTE_EINVAL
    out = np.zeros(4, dtype=np.uint8)
    assert lib.lte_plan_turbo_iters_used(None, C.ptr(out, C.U8), 4) == C.LTE_EINVAL


def test_run_grid_keyword():
    import lte_phy
    params = list(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters.values())
    assert params[-1].name == 'early_stop' and params[-1].default is False


def test_run_grid_refuses_early_stop_where_nothing_is_decoded():
    """Raised from the keyword check, before any plan (or device) is needed."""
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    for kw in (dict(coded=False), dict(coded=False, mimo='sfbc'), dict(coded=False, mimo='spatial'),
               dict(coded=False, mimo='beamforming'), dict(coded=False, num_rx=2)):
        with pytest.raises(ValueError, match='early_stop'):
            sim.run_grid([0.0], 1, early_stop=True, **kw)


def test_plan_keyword():
    from lte_phy import engine
    p = inspect.signature(engine.Plan.__init__).parameters['early_stop']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_channel_coding_entry_is_not_a_reference_name():
    from lte_phy import channel_coding
    assert callable(channel_coding.turbo_decode_early_stop)
    assert 'turbo_decode_early_stop' not in channel_coding.__all__ and len(channel_coding.__all__) == 18
    sig = inspect.signature(channel_coding.turbo_decode_early_stop)
    assert sig.parameters['max_iterations'].default == 8 and sig.parameters['crc'].default == '24B'
    with pytest.raises(ValueError):
        channel_coding.turbo_decode_early_stop(np.zeros(132), 40, crc='16')
