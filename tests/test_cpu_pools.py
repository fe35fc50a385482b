"""The rules of the two pools as pure functions, through tests/hostlib/pool_print.cc, a plain C++ program: which cached
block serves a request and what becomes of a block that is given back (zopfli_amd/csrc/device/zmx_pool_rules.h), and
which contexts a call takes (zopfli_amd/csrc/host/deal.h: ChooseSlots).  CPU only; integers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_PRINT = os.path.join(ROOT, "tests", "_build", "pool_print")
MIB = 1 << 20


@pytest.fixture(scope="module")
def pool():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "pool_print"])

    def run(*args):
        out = subprocess.run([POOL_PRINT] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
        return [[int(x) for x in line.split()] for line in out.splitlines()]
    return run


def fit(pool, which, want, caps):
    return pool("fit", which, want, ",".join(str(c) for c in caps) or "-")[0][0]


def test_best_fit_of_nothing(pool):
    assert fit(pool, "device", 1000, []) == -1
    assert fit(pool, "pinned", 1000, []) == -1


def test_best_fit_takes_an_equal_capacity(pool):
    assert fit(pool, "device", 1000, [1000]) == 0
    assert fit(pool, "device", 1000, [999]) == -1


@pytest.mark.parametrize("want", [1, 1000, 3 * MIB + 5])
def test_best_fit_device_bound(pool, want):
    """A cached block of up to 2 * want + 1 MiB serves, one byte more does not."""
    assert fit(pool, "device", want, [2 * want + MIB]) == 0
    assert fit(pool, "device", want, [2 * want + MIB + 1]) == -1
    assert fit(pool, "device", want, [2 * want + MIB + 1, 2 * want + MIB]) == 1


@pytest.mark.parametrize("caps,want_index", [([5000, 3000, 4000], 1), ([3000, 4000, 5000], 0), ([5000, 4000, 3000], 2),
                                             ([900, 4000, 10 * MIB, 3500], 3), ([3000, 3000], 0)])
def test_best_fit_takes_the_smallest_that_fits(pool, caps, want_index):
    assert fit(pool, "device", 1000, caps) == want_index


@pytest.mark.parametrize("want", [1, 4096, 100000])
def test_best_fit_pinned_bound(pool, want):
    """A cached pinned buffer of up to 4 * bytes + 4096 serves, one byte more does not."""
    assert fit(pool, "pinned", want, [4 * want + 4096]) == 0
    assert fit(pool, "pinned", want, [4 * want + 4097]) == -1
    assert fit(pool, "pinned", want, [want - 1]) == -1
    # (between the two bounds: the pinned list takes what the device list refuses)
    assert fit(pool, "pinned", MIB, [4 * MIB]) == 0 and fit(pool, "device", MIB, [4 * MIB]) == -1


def test_pinned_constants(pool):
    assert pool("pinned") == [[4096, 8, 64 * MIB]]


def free(pool, device_cached, own_cached, cap, keep):
    (trim_others, cache), = pool("free", device_cached, own_cached, cap, keep)
    return bool(trim_others), bool(cache)


def test_free_below_the_budget_is_cached(pool):
    assert free(pool, 0, 0, 100, 1000) == (False, True)
    assert free(pool, 500, 200, 100, 1000) == (False, True)      # another context's 300 beside it: still no hook
    assert free(pool, 900, 900, 100, 1000) == (False, True)      # exactly the budget


def test_free_over_a_budget_that_is_all_its_own(pool):
    assert free(pool, 901, 901, 100, 1000) == (False, False)
    assert free(pool, 0, 0, 1001, 1000) == (False, False)


def test_free_over_a_budget_that_others_share(pool):
    """The hook first; what it left decides between the cache and the device."""
    assert free(pool, 950, 400, 100, 1000) == (True, False)
    assert free(pool, 400, 400, 100, 1000) == (False, True)      # asked again: the others' 550 are gone
    assert free(pool, 950, 949, 100, 1000) == (True, False)
    assert free(pool, 949, 949, 100, 1000) == (False, False)     # asked again: one byte went, the block still does not fit


def slots(pool, want, per_device, small, may_create_more, devices, lanes=3, small_lanes=16):
    picks = pool("slots", want, per_device, int(small), int(may_create_more), lanes, small_lanes, *devices)
    assert len({(d, s) for d, s, _ in picks}) == len(picks), "a slot was chosen twice"
    return [tuple(p) for p in picks]


def test_slots_first_context(pool):
    assert slots(pool, 1, 1, False, True, ["0:"]) == [(0, 0, 1)]


def test_slots_polite_call_creates_one(pool):
    assert slots(pool, 1, 3, False, False, ["0:"]) == [(0, 0, 1)]
    # ... but takes what exists and is free
    assert slots(pool, 1, 3, False, False, ["0:ff"]) == [(0, 0, 0), (0, 1, 0)]
    assert slots(pool, 1, 3, False, False, ["0:bb"]) == [(0, 2, 1)]


def test_slots_may_create_more(pool):
    assert slots(pool, 1, 3, False, True, ["0:"]) == [(0, 0, 1), (0, 1, 1), (0, 2, 1)]
    assert slots(pool, 1, 3, False, True, ["0:bf"]) == [(0, 1, 0), (0, 2, 1)]
    assert slots(pool, 1, 4, False, True, ["0:"]) == [(0, 0, 1), (0, 1, 1), (0, 2, 1)]     # not past `lanes`


def test_slots_small_call_grows_the_first_live_device(pool):
    """Every one of `lanes` busy: a small call gets one more on the FIRST live device, up to small_lanes, before the
    next device is looked at (ADVICE.md item 1 describes this; the policy is kept)."""
    assert slots(pool, 1, 1, True, True, ["0:bbb", "1:"]) == [(0, 3, 1)]
    assert slots(pool, 1, 1, True, True, ["0:" + "b" * 15, "1:"]) == [(0, 15, 1)]
    assert slots(pool, 1, 1, True, True, ["0:" + "b" * 16, "1:"]) == [(1, 0, 1)]
    assert slots(pool, 1, 1, True, True, ["0!:", "1:bbb", "2:"]) == [(1, 3, 1)]
    assert slots(pool, 1, 1, False, True, ["0:bbb", "1:"]) == [(1, 0, 1)]                   # not small: the next device
    assert slots(pool, 1, 1, True, True, ["0:bbb"], small_lanes=3) == []


def test_slots_small_call_with_several_per_device_stays_within_lanes(pool):
    assert slots(pool, 1, 3, True, True, ["0:bbb"]) == []
    assert slots(pool, 1, 3, True, True, ["0:bb"]) == [(0, 2, 1)]
    assert slots(pool, 1, 2, True, True, ["0:bfb"]) == [(0, 1, 0)]


def test_slots_skip_a_dead_device(pool):
    assert slots(pool, 1, 1, False, True, ["0!:", "1:"]) == [(1, 0, 1)]
    assert slots(pool, 2, 1, False, True, ["0:f", "1!:f", "2:f"]) == [(0, 0, 0), (2, 0, 0)]
    assert slots(pool, 1, 1, False, True, ["0!:", "1!:"]) == []


def test_slots_stop_at_the_wanted_devices(pool):
    assert slots(pool, 2, 1, False, True, ["0:", "1:", "2:"]) == [(0, 0, 1), (1, 0, 1)]
    assert slots(pool, 2, 2, False, True, ["0:f", "1:bbb", "2:ff", "3:f"]) == [(0, 0, 0), (0, 1, 1), (2, 0, 0), (2, 1, 0)]


def test_slots_nothing_free_and_nothing_to_create(pool):
    assert slots(pool, 3, 2, False, True, ["0:bbb", "1:bnb"]) == []
    assert slots(pool, 1, 1, False, True, []) == []


def test_slots_never_twice(pool):
    """Every lane of a device gets a slot of its own, an existing one or a new one (checked for every answer above too)."""
    picks = slots(pool, 3, 3, False, True, ["0:fbf", "1:f", "2:"])
    assert picks == [(0, 0, 0), (0, 2, 0), (1, 0, 0), (1, 1, 1), (1, 2, 1), (2, 0, 1), (2, 1, 1), (2, 2, 1)]
