"""CPU: what kind of chain each chain value is (lte_chain_info, the one table of
csrc/lte_chain.h as Python sees it), and every refusal lte_plan_create /
lte_plan_create_harq make from it before the device is touched, held to the
outcomes recorded in tests/golden/plan_create_refusals.json."""
import ctypes
import itertools
import json
import os

import pytest

from conftest import ROOT

REFUSALS = os.path.join(ROOT, 'tests', 'golden', 'plan_create_refusals.json')

# lte_chain_info's fields
SISO, MIMO, BF = 0, 1, 2                       # family: run_siso / run_mimo / run_bf
NONE, SFBC, SPATIAL = -1, 0, 1                 # mode
NEVER, FLAG, ALWAYS = 0, 1, 2                  # precode: never / follows desc.sc_fdm / always

# chain value -> (family, coded, mode, precode)
EXPECTED = {
    0: (SISO, 0, NONE, FLAG),       # LTE_CHAIN_UNCODED
    1: (SISO, 1, NONE, NEVER),      # LTE_CHAIN_CODED
    2: (SISO, 0, NONE, FLAG),       # LTE_CHAIN_SIMO
    3: (MIMO, 0, SFBC, NEVER),      # LTE_CHAIN_SFBC
    4: (MIMO, 1, SFBC, NEVER),      # LTE_CHAIN_SFBC_CODED
    5: (MIMO, 0, SPATIAL, NEVER),   # LTE_CHAIN_SPATIAL
    6: (BF, 0, NONE, NEVER),        # LTE_CHAIN_BEAMFORMING
    7: (SISO, 1, NONE, NEVER),      # LTE_CHAIN_SIMO_CODED
    8: (MIMO, 1, SPATIAL, NEVER),   # LTE_CHAIN_SPATIAL_CODED
    9: (SISO, 1, NONE, ALWAYS),     # LTE_CHAIN_SCFDM_CODED
}


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


@pytest.mark.parametrize('chain', sorted(EXPECTED))
def test_chain_classification(C, chain):
    """(family, coded, mode, precode) of every chain value, literally.  The table
    implies what the per-chain host tests used to pin as sets: the coded chains
    among 0..7 are {1, 4, 7} and the multi-antenna ones {3, 4, 5}; 8 is both coded
    and multi-antenna; 9 is coded and not multi-antenna; 0 is uncoded.  Plan.coded
    / Plan.mimo (engine.chain_is_coded / chain_is_mimo) give the same answers, and
    a value next to the range is refused as a bad chain."""
    from lte_phy import engine
    family, coded, mode, precode = EXPECTED[chain]
    assert tuple(C.chain_info(chain)) == (family, coded, mode, precode)
    assert engine.chain_is_coded(chain) is bool(coded)
    assert engine.chain_is_mimo(chain) is (family == MIMO)
    assert len(EXPECTED) == 10
    for bad in (-1, 10):
        with pytest.raises(ValueError, match='bad chain'):
            C.chain_info(bad)
        info = (ctypes.c_int32 * 4)()
        assert C.load().lte_chain_info(bad, info, 4) == C.LTE_EINVAL
        assert b'bad chain' in C.load().lte_last_error()


# ---------------------------------------------------------------- refusals
CHAINS, NUM_TX, NUM_RX = range(-1, 11), (0, 1, 2, 3, 4, 8), (0, 1, 2, 5, 9, 17)
DETECTORS, RANKS = range(0, 5), range(0, 4)
HARQ_CHAINS, HARQ_NUM_RX = range(0, 10), (1, 2)


def _desc(C, chain, num_tx, num_rx, detector, rank):
    d = C.PlanDesc()
    d.N, d.Nc, d.cp_len, d.bps, d.n_bits, d.n_sym, d.max_frames = 128, 72, 9, 2, 100, 2, 1
    d.channel = C.CH_AWGN
    d.chain, d.num_tx, d.num_rx, d.detector, d.rank = chain, num_tx, num_rx, detector, rank
    return d


def _outcome(C, rc, h):
    """(code, message) of a refusal made from the descriptor; None for a
    descriptor that passed those checks (a plan, destroyed at once, or a device /
    allocation failure where there is no device)."""
    lib = C.load()
    if rc in (C.LTE_EINVAL, C.LTE_EUNSUP):
        return [rc, lib.lte_last_error().decode()]
    if rc == C.LTE_OK:
        lib.lte_plan_destroy(h)
    return None


def sweep(C):
    """The outcomes of both sweeps, in sweep order."""
    lib = C.load()
    create, create_harq = [], []
    for chain, num_tx, num_rx, detector, rank in itertools.product(CHAINS, NUM_TX, NUM_RX, DETECTORS, RANKS):
        d, h = _desc(C, chain, num_tx, num_rx, detector, rank), ctypes.c_void_p()
        create.append(_outcome(C, lib.lte_plan_create(ctypes.byref(d), ctypes.byref(h)), h))
    for chain, num_rx in itertools.product(HARQ_CHAINS, HARQ_NUM_RX):
        d, hd, h = _desc(C, chain, 1, num_rx, 0, 0), C.HarqDesc(), ctypes.c_void_p()
        hd.max_tx = 2
        create_harq.append(_outcome(C, lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)), h))
    return create, create_harq


def pack(create, create_harq):
    """The fixture's form: the distinct outcomes once, one index per descriptor."""
    outcomes = []
    for o in create + create_harq:
        if o not in outcomes:
            outcomes.append(o)
    return {'outcomes': outcomes, 'create': [outcomes.index(o) for o in create],
            'create_harq': [outcomes.index(o) for o in create_harq]}


def test_plan_create_refusals_match_the_recorded_ones(C):
    """Every descriptor of the sweep gets the return code and lte_last_error()
    text recorded from the library before the chain table existed, including
    which refusal wins where several apply."""
    want = json.load(open(REFUSALS))
    create, create_harq = sweep(C)
    assert len(create) == 12 * 6 * 6 * 5 * 4 == len(want['create'])
    assert len(create_harq) == 20 == len(want['create_harq'])
    keys = list(itertools.product(CHAINS, NUM_TX, NUM_RX, DETECTORS, RANKS))
    diff = [(k, got, want['outcomes'][i]) for k, got, i in zip(keys, create, want['create'])
            if got != want['outcomes'][i]]
    assert not diff, (len(diff), diff[:5])
    keys = list(itertools.product(HARQ_CHAINS, HARQ_NUM_RX))
    diff = [(k, got, want['outcomes'][i]) for k, got, i in zip(keys, create_harq, want['create_harq'])
            if got != want['outcomes'][i]]
    assert not diff, diff
