"""CPU: the interface of the coded SIMO chain (LTE_CHAIN_SIMO_CODED: 1 x N MRC
with turbo coding) -- the header line, the ctypes constant, the ABI version,
the checks lte_plan_create_harq makes before the device is touched, the Python
entry point's signature, and the model of tests/simo_coded_model.py on its own:
every ladder case of tests/test_gpu_simo_coded.py straddles the turbo cliff, so
an agreement there says something.  The kernels are checked on the GPU in
tests/test_gpu_simo_coded.py."""
import inspect
import os
import re

import pytest

from conftest import ROOT
import simo_coded_model as M


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def test_header_and_binding_name_the_chain(C):
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    assert re.search(r'^\s*LTE_CHAIN_SIMO_CODED = 7$', text, re.M)
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)      # an additive value: no new version
    assert C.CHAIN_SIMO_CODED == 7
    assert len({C.CHAIN_UNCODED, C.CHAIN_CODED, C.CHAIN_SIMO, C.CHAIN_SFBC, C.CHAIN_SFBC_CODED, C.CHAIN_SPATIAL,
                C.CHAIN_BEAMFORMING, C.CHAIN_SIMO_CODED}) == 8


def test_abi_version_is_unchanged(C):
    assert C.load().lte_version() == 3 and C.ABI_VERSION == 3


def test_create_harq_refuses_the_chain_without_a_device(C):
    import ctypes
    lib = C.load()
    d, hd, h = C.PlanDesc(), C.HarqDesc(), ctypes.c_void_p()
    d.chain, d.num_rx, hd.max_tx = C.CHAIN_SIMO_CODED, 2, 4
    assert lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)) == C.LTE_EUNSUP
    assert b'HARQ' in lib.lte_last_error()


def test_plan_create_knows_the_chain_without_a_device(C):
    """Chain 7 passes the chain-range check (the next refusal, of num_rx = 0, is
    reached) and chain 8 does not."""
    import ctypes
    lib = C.load()
    d, h = C.PlanDesc(), ctypes.c_void_p()
    d.N, d.Nc, d.cp_len, d.bps, d.num_rx, d.n_bits, d.max_frames = 128, 72, 9, 2, 0, 100, 1
    d.chain = C.CHAIN_SIMO_CODED
    assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EINVAL
    assert b'num_rx' in lib.lte_last_error()
    d.chain = 8
    assert lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)) == C.LTE_EINVAL
    assert b'bad chain' in lib.lte_last_error()


def test_plan_classifies_the_chain_as_coded_siso_family(C):
    """(Every chain's classification, the other chains' included: tests/test_chain_traits_host.py.)"""
    from lte_phy import engine
    assert engine.chain_is_coded(C.CHAIN_SIMO_CODED)            # Plan.coded
    assert not engine.chain_is_mimo(C.CHAIN_SIMO_CODED)         # Plan.mimo: one TX, the SISO capture shapes
    assert C.chain_info(C.CHAIN_SIMO_CODED).family == C.FAMILY_SISO


def test_simulate_simo_coded_signature_and_refusal():
    import lte_phy
    sig = inspect.signature(lte_phy.OFDMSimulator.simulate_simo_coded)
    got = [(p.name, p.default) for p in sig.parameters.values()][1:]
    assert got == [('bits', inspect.Parameter.empty), ('snr_db', 10.0), ('num_rx', 2)]
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    with pytest.raises(ValueError, match='num_rx must be >= 1'):
        sim.simulate_simo_coded([0, 1, 1, 0], 5.0, num_rx=0)
    with pytest.raises(ValueError, match='cannot be empty'):
        sim.simulate_simo_coded([], 5.0)
    grid = list(inspect.signature(lte_phy.OFDMSimulator.run_grid).parameters)
    assert grid[:6] == ['self', 'snr_range', 'num_trials', 'seed', 'coded', 'num_rx'] and len(grid) == 17
    with pytest.raises(ValueError, match='coded SISO'):         # HARQ stays on the coded SISO chain
        sim.run_harq_grid([0.0], 1, n_bits=435, num_rx=2)


def test_model_deinterleave_is_the_oracles(oracle):
    num = oracle.Numerology(bandwidth=1.25, modulation='QPSK')
    perm, rows, total = oracle.tf_interleave_perm(700, num.Nd)
    src = M.deinterleave_index(700, num.Nd)
    # interleaved[j] = padded[perm[j]] lands on RE j: coded symbol q sits where perm == q
    import numpy as np
    inv = np.empty(total, dtype=int)
    inv[perm] = np.arange(total)
    assert np.array_equal(src, inv[:700])


@pytest.mark.parametrize('name', list(M.CASES))
def test_ladder_case_straddles_the_cliff(oracle, name):
    """The model alone, 67 frames at 2 iterations: at least 8 frames pass their
    CRC and at least 8 fail, so the frames' decisions react to a wrong LLR."""
    inp, frames = M.case_frames(oracle, name)
    ok = [f['crc'] for f in frames]
    n_ok = sum(ok)
    print(f'simo coded ladder {name}: {n_ok} pass / {M.FRAMES - n_ok} fail over {M.CASES[name]["snr"]} dB')
    assert len(ok) == M.FRAMES == 67
    assert n_ok >= M.MIN_PASS and M.FRAMES - n_ok >= M.MIN_FAIL, (name, n_ok)
    assert all((f['errs'] == 0) == f['crc'] for f in frames)    # (no CRC false alarm in the ladder)
