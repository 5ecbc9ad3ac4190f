"""GPU: the library frees every device buffer it allocates.

lte_device_bytes_held() is the library's own count of the bytes its device
buffers hold in this process (device-wide free memory would also move with
other processes' work).  Every assertion here is an equality on that count:

  (1) a plan of each chain family, created, run once and destroyed, leaves it
      where it was (f32 and f64; one code block and two)
  (2) a plan lte_plan_create refuses leaves it where it was, whatever had been
      uploaded by then
  (3) runs with captures grow a plan's buffers once, in the first run, and the
      capture temporaries are gone after each run

All at the smallest numerology (N = 128) with max_frames = 65: two 64-frame
decoder groups.  Only argument errors and plain successful runs are used."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 65
RAY = dict(delays=(0, 1, 3), gains=(0.8, 0.5, 0.3))


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


def held(C):
    gc.collect()   # plans other tests dropped go now, not between two readings
    return int(C.load().lte_device_bytes_held())


def base(C, **kw):
    d = dict(N=128, Nc=72, cp_len=9, bps=2, n_sym=0, chain=C.CHAIN_CODED, channel=C.CH_AWGN, fs=1.92e6, n_bits=40,
             max_frames=FRAMES)
    d.update(kw)
    return d


def families(C):
    """name -> Plan keywords; the coded ones carry 40 bits (one code block, K = 64)."""
    return {
        'uncoded': base(C, chain=C.CHAIN_UNCODED, n_sym=2, n_bits=100),
        'coded-harq': base(C, harq=dict(max_tx=2, rv_seq=(0, 2))),
        'coded-early-stop': base(C, early_stop=True),          # (HARQ plans refuse early stop: its own plan)
        'coded-2cb': base(C, bps=4, n_bits=6200, channel=C.CH_RAYLEIGH, **RAY),   # two code blocks
        'coded-2cb-early-stop': base(C, n_bits=6200, early_stop=True),
        'simo-coded-1x2': base(C, chain=C.CHAIN_SIMO_CODED, num_rx=2, channel=C.CH_RAYLEIGH, **RAY),
        'sfbc-coded-2x2': base(C, chain=C.CHAIN_SFBC_CODED, num_tx=2, num_rx=2, channel=C.CH_RAYLEIGH, **RAY),
        'spatial-2x2': base(C, chain=C.CHAIN_SPATIAL, num_tx=2, num_rx=2, n_sym=2, n_bits=200),
        'beamforming-2x1': base(C, chain=C.CHAIN_BEAMFORMING, num_tx=2, num_rx=1, n_sym=2, n_bits=100),
    }


FAMILY_NAMES = ['uncoded', 'coded-harq', 'coded-early-stop', 'coded-2cb', 'coded-2cb-early-stop', 'simo-coded-1x2',
                'sfbc-coded-2x2', 'spatial-2x2', 'beamforming-2x1']


def destroy(C, plan):
    assert C.load().lte_plan_destroy(plan.h) == C.LTE_OK
    plan.h = None


# ---------------------------------------------------------------------------
# (1) create, run, destroy
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_create_run_destroy_returns_every_byte(C, family, prec):
    from lte_phy import engine
    kw = families(C)[family]
    start = held(C)
    plan = engine.Plan(precision=prec, **kw)
    assert held(C) > start
    if plan.harq is not None:
        plan.harq_round(0)
    r = plan.run(np.full(FRAMES, 8.0), seed=5)
    assert int(r['counts'][0, 3]) == FRAMES          # every frame went through the chain
    if '2cb' in family:
        assert plan.n_cb == 2
    destroy(C, plan)
    assert held(C) == start


# ---------------------------------------------------------------------------
# (2) refused plans
def refused(C, **kw):
    """lte_plan_create's (code, message) for Plan keywords it refuses."""
    d = C.PlanDesc()
    for k, v in kw.items():
        if k in ('delays', 'gains'):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
            d.n_paths = len(v)
        else:
            setattr(d, k, v)
    h = ctypes.c_void_p()
    rc = C.load().lte_plan_create(ctypes.byref(d), ctypes.byref(h))
    assert not h.value
    return rc, C.load().lte_last_error().decode()


def test_refused_plans_free_what_they_uploaded(C):
    uncoded = dict(N=128, Nc=72, cp_len=9, bps=2, chain=C.CHAIN_UNCODED, channel=C.CH_AWGN, num_rx=1, fs=1.92e6,
                   max_frames=FRAMES)
    from lte_phy import engine
    probe = engine.Plan(n_sym=2, n_bits=1, **uncoded)
    Nd = probe.Nd                     # data subcarriers per OFDM symbol, as the library lays the grid out
    destroy(C, probe)
    start = held(C)
    # one bit more than n_sym * Nd * bps: refused after the grid tables went up
    rc, msg = refused(C, n_sym=2, n_bits=2 * Nd * 2 + 1, **uncoded)
    assert rc == C.LTE_EINVAL and msg == 'n_bits exceeds frame capacity'
    assert held(C) == start
    rc, msg = refused(C, n_sym=0, n_bits=10, **uncoded)
    assert rc == C.LTE_EINVAL and msg == 'n_sym must be >= 1'
    assert held(C) == start
    # the tables, then the delays are looked at
    rc, msg = refused(C, n_sym=2, n_bits=10, **dict(uncoded, channel=C.CH_RAYLEIGH), delays=(0, -1, 3),
                      gains=RAY['gains'])
    assert rc == C.LTE_EINVAL and msg == 'negative delay'
    assert held(C) == start


# ---------------------------------------------------------------------------
# (3) captures do not accumulate
@pytest.mark.parametrize('family,capture', [('sfbc-coded-2x2', ('link_stats', 'signal_rx')),
                                            ('coded-2cb', ('signal_rx',))])
def test_captures_do_not_accumulate(C, family, capture):
    from lte_phy import engine
    start = held(C)
    plan = engine.Plan(**families(C)[family])
    after = []
    for i in range(3):
        r = plan.run(np.full(FRAMES, 8.0), seed=5 + i, capture=capture)
        assert all(np.any(r[k] != 0) for k in capture)
        after.append(held(C))
    assert after[1] == after[2]       # the first run did all the growing
    destroy(C, plan)
    assert held(C) == start
