"""The device layer's switches (zopfli_amd/csrc/device/zmx_knobs.h) and the host layer's (zopfli_amd/csrc/host/host_knobs.h:
the process table and the pool table): tests/hostlib/knob_print.cc parses this process's environment with the headers'
own functions and prints the structs; the defaults and the odd inputs of every switch whose text is not taken as it
stands.  Also: every ZOPFLI_AMD_* / ZOPFLIPNG_AMD_* name the sources read is in
the table of INTEGRATION.md, and the table names nothing else.  CPU only; integer and string equality."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB_PRINT = os.path.join(ROOT, "tests", "_build", "knob_print")

DEFAULTS = {
    "guard": "0", "guard_selftest": "0", "prof": "0", "kernel_timing": "0", "bc_prof": "0",
    "match": "0", "match_order": "1", "match_filter": "1", "match_hits": "300", "pool_entries": "0",
    "run_codes": "0", "code_budget_mb": "0",
    "seg_l_set": "0", "seg_l": "4096", "seg_head": "0", "seg_warm": "512", "seg_cuts": "1024", "seg_mid": "1",
    "seg_redo": "1", "seg_scale": "1", "seg_debug": "0", "fix_lean": "-1", "int_path": "1", "shortcut_chain": "1",
}


@pytest.fixture(scope="module")
def knobs():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "knob_print"])

    def run(*mode, **env):
        """The parsed struct as {field: text} with only ZOPFLI_AMD_<KEY>=value of `env` set (LOCAL_RANK as it stands);
        `mode`: nothing = the device table, "host", or "pool", N."""
        clean = {k: v for k, v in os.environ.items() if not k.startswith("ZOPFLI_AMD_") and k != "LOCAL_RANK"}
        clean.update({k if k == "LOCAL_RANK" else "ZOPFLI_AMD_" + k: str(v) for k, v in env.items()})
        out = subprocess.run([KNOB_PRINT] + [str(m) for m in mode], env=clean, capture_output=True, text=True,
                             check=True).stdout
        return dict(line.split("=", 1) for line in out.splitlines())
    return run


def test_defaults(knobs):
    assert knobs() == DEFAULTS


@pytest.mark.parametrize("text,want", [("0", "0"), ("2", "2"), ("3", "2"), ("4", "2"), ("5", "5"), ("7", "2"), ("-1", "2")])
def test_match_kernel(knobs, text, want):
    """0 and 5 are kept; everything else, the removed kernels 3 and 4 included, selects kernel 2."""
    assert knobs(MATCH=text) == dict(DEFAULTS, match=want)


@pytest.mark.parametrize("text,want", [("0", "0"), ("100", "64"), ("4096", "4096")])
def test_seg_l(knobs, text, want):
    assert knobs(SEG_L=text) == dict(DEFAULTS, seg_l=want, seg_l_set="1")


@pytest.mark.parametrize("text,want", [("1", "64"), ("65", "128"), (str(2 ** 21), str(2 ** 20))])
def test_seg_warm(knobs, text, want):
    assert knobs(SEG_WARM=text) == dict(DEFAULTS, seg_warm=want)


def test_seg_head_is_a_multiple_of_64(knobs):
    assert knobs(SEG_HEAD="4100") == dict(DEFAULTS, seg_head="4096")


def test_match_hits_is_not_negative(knobs):
    assert knobs(MATCH_HITS="-5") == dict(DEFAULTS, match_hits="0")
    assert knobs(MATCH_HITS="17") == dict(DEFAULTS, match_hits="17")


@pytest.mark.parametrize("field,key", [("guard", "GUARD"), ("run_codes", "RUN_CODES")])
@pytest.mark.parametrize("text,want", [("0", "0"), ("x", "0"), ("1", "1")])
def test_on_only_for_a_non_zero_integer(knobs, field, key, text, want):
    assert knobs(**{key: text}) == dict(DEFAULTS, **{field: want})


def test_kernel_timing_falls_back_to_prof(knobs):
    assert knobs()["kernel_timing"] == "0"
    assert knobs(PROF="1") == dict(DEFAULTS, prof="1", kernel_timing="1")
    assert knobs(PROF="") == dict(DEFAULTS, prof="1", kernel_timing="1")            # set at all
    assert knobs(PROF="1", KERNEL_TIMING="0") == dict(DEFAULTS, prof="1", kernel_timing="0")
    assert knobs(KERNEL_TIMING="1") == dict(DEFAULTS, kernel_timing="1")


def test_other_values(knobs):
    assert knobs(SEG_REDO="0", FIX_LEAN="0", SEG_SCALE="1.9", CODE_BUDGET_MB="0", SEG_CUTS="70000", SEG_MID="0",
                 MATCH_ORDER="0", MATCH_FILTER="0", POOL_ENTRIES="2000", GUARD_SELFTEST="7", BC_PROF="1") == dict(
        DEFAULTS, seg_redo="0", fix_lean="0", seg_scale="1.89999998", code_budget_mb="1", seg_cuts="65536",
        seg_mid="0", match_order="0", match_filter="0", pool_entries="2000", guard_selftest="7", bc_prof="1")


# ---- the host layer's process table: every reading rule as the code before the table read it

HOST_DEFAULTS = {
    "split_mb": "-1", "split_ways": "3", "split_runs": "1", "stream_prio": "1", "small_prio": "1", "upload_order": "1",
    "deal_by_cost": "1", "shard_weights": "", "deal_after": "8", "round_parts": "2000", "parts_per_batch": "256",
    "test_fail_shard": "-1", "keep_heap": "0", "batch_split": "-1", "device_split": "1", "device_split_from": "-1",
    "device_split_min": "128", "device_encode": "1", "verify": "0", "trace_call": "0", "prof": "0",
    "threads": "0", "threads_set": "0", "wide_threads": "0", "host_cache_mb": "1024", "host_cache_min": "32768",
}


def host_case(knobs, want, **env):
    assert knobs("host", **env) == dict(HOST_DEFAULTS, **want), env


def test_host_defaults(knobs):
    assert knobs("host") == HOST_DEFAULTS


def test_host_split(knobs):
    """SPLIT_MB unset = -1, "by the options"; a negative text = 0 = never.  SPLIT_WAYS is at least 1."""
    host_case(knobs, {"split_mb": "2"}, SPLIT_MB="2")
    host_case(knobs, {"split_mb": "0"}, SPLIT_MB="0")
    host_case(knobs, {"split_mb": "0"}, SPLIT_MB="-4")
    host_case(knobs, {"split_ways": "1"}, SPLIT_WAYS="0")
    host_case(knobs, {"split_ways": "1"}, SPLIT_WAYS="-2")
    host_case(knobs, {"split_ways": "5"}, SPLIT_WAYS="5")


def test_host_counts_fall_back_when_not_positive(knobs):
    host_case(knobs, {"round_parts": "2000"}, ROUND_PARTS="0")
    host_case(knobs, {"round_parts": "2000"}, ROUND_PARTS="-1")
    host_case(knobs, {"round_parts": "2"}, ROUND_PARTS="2")
    host_case(knobs, {"parts_per_batch": "256"}, PARTS_PER_BATCH="0")
    host_case(knobs, {"parts_per_batch": "256"}, PARTS_PER_BATCH="-7")
    host_case(knobs, {"parts_per_batch": "1"}, PARTS_PER_BATCH="1")


def test_host_deal(knobs):
    """Only the text "count" turns the cost dealing off."""
    host_case(knobs, {"deal_by_cost": "0"}, DEAL="count")
    host_case(knobs, {"deal_by_cost": "1"}, DEAL="cost")
    host_case(knobs, {"deal_by_cost": "1"}, DEAL="")
    host_case(knobs, {"deal_by_cost": "1"}, DEAL="0")


def test_host_device_split(knobs):
    host_case(knobs, {"device_split": "0"}, DEVICE_SPLIT="0")
    host_case(knobs, {"device_split": "1"}, DEVICE_SPLIT="1")
    host_case(knobs, {"device_split": "2"}, DEVICE_SPLIT="2")
    host_case(knobs, {"device_split_from": "0"}, DEVICE_SPLIT_FROM="0")     # 0 is a threshold; unset (-1) = the caller's
    host_case(knobs, {"device_split_from": "1"}, DEVICE_SPLIT_FROM="1")
    host_case(knobs, {"device_split_min": "0"}, DEVICE_SPLIT_MIN="0")
    host_case(knobs, {"device_split_min": "7"}, DEVICE_SPLIT_MIN="7")


def test_host_batch_split(knobs):
    """Unset = -1 = by the number of parts; 0 and 1 force."""
    host_case(knobs, {"batch_split": "0"}, BATCH_SPLIT="0")
    host_case(knobs, {"batch_split": "1"}, BATCH_SPLIT="1")


@pytest.mark.parametrize("field,key", [("device_encode", "DEVICE_ENCODE"), ("upload_order", "UPLOAD_ORDER"),
                                       ("small_prio", "SMALL_PRIO"), ("split_runs", "SPLIT_RUNS")])
@pytest.mark.parametrize("text,want", [("1", "1"), ("0", "0"), ("x", "0"), ("", "0")])
def test_host_on_unless_zero(knobs, field, key, text, want):
    """Default on; any text that is no non-zero integer turns it off."""
    host_case(knobs, {field: want}, **{key: text})


@pytest.mark.parametrize("text", ["0", "1", "2"])
def test_host_stream_prio(knobs, text):
    host_case(knobs, {"stream_prio": text}, STREAM_PRIO=text)


@pytest.mark.parametrize("field,key", [("trace_call", "TRACE_CALL"), ("verify", "VERIFY")])
@pytest.mark.parametrize("text,want", [("1", "1"), ("3", "1"), ("0", "0"), ("x", "0"), ("", "0")])
def test_host_on_only_for_a_non_zero_integer(knobs, field, key, text, want):
    host_case(knobs, {field: want}, **{key: text})


def test_host_prof_is_on_when_set_at_all(knobs):
    host_case(knobs, {"prof": "1"}, PROF="1")
    host_case(knobs, {"prof": "1"}, PROF="0")
    host_case(knobs, {"prof": "1"}, PROF="")


@pytest.mark.parametrize("text,want", [("0", "0"), ("1", "1"), ("2", "2"), ("3", "1"), ("x", "0")])
def test_host_keep_heap(knobs, text, want):
    """0 = malloc is left alone, 2 = the settings for measuring, any other integer the plain ones."""
    host_case(knobs, {"keep_heap": want}, KEEP_HEAP=text)


def test_host_cache(knobs):
    host_case(knobs, {"host_cache_mb": "0"}, HOST_CACHE_MB="0")
    host_case(knobs, {"host_cache_mb": "0"}, HOST_CACHE_MB="-5")
    host_case(knobs, {"host_cache_mb": "64"}, HOST_CACHE_MB="64")
    host_case(knobs, {"host_cache_min": "1024"}, HOST_CACHE_MIN="10")
    host_case(knobs, {"host_cache_min": "1024"}, HOST_CACHE_MIN="-1")
    host_case(knobs, {"host_cache_min": "4096"}, HOST_CACHE_MIN="4096")


def test_host_threads(knobs):
    """A positive THREADS / WIDE_THREADS is taken; THREADS set at all makes the wide pool as wide as the regular one
    (threads_set), also where its value is not taken."""
    host_case(knobs, {"threads": "8", "threads_set": "1"}, THREADS="8")
    host_case(knobs, {"threads": "0", "threads_set": "1"}, THREADS="0")
    host_case(knobs, {"threads": "0", "threads_set": "1"}, THREADS="-2")
    host_case(knobs, {"wide_threads": "24"}, WIDE_THREADS="24")
    host_case(knobs, {"wide_threads": "0"}, WIDE_THREADS="0")
    host_case(knobs, {"threads": "8", "threads_set": "1", "wide_threads": "24"}, THREADS="8", WIDE_THREADS="24")


def test_host_test_hooks(knobs):
    host_case(knobs, {"test_fail_shard": "1"}, TEST_FAIL_SHARD="1")
    host_case(knobs, {"test_fail_shard": "0"}, TEST_FAIL_SHARD="0")
    host_case(knobs, {"deal_after": "0"}, DEAL_AFTER="0")
    host_case(knobs, {"deal_after": "0"}, DEAL_AFTER="-3")
    host_case(knobs, {"deal_after": "20"}, DEAL_AFTER="20")


def test_host_shard_weights(knobs):
    """Numbers separated by commas, read up to the first text that is no number; a negative weight counts as 0."""
    host_case(knobs, {"shard_weights": "28,36,36"}, SHARD_WEIGHTS="28,36,36")
    host_case(knobs, {"shard_weights": "1"}, SHARD_WEIGHTS="1,,2")
    host_case(knobs, {"shard_weights": "0,1"}, SHARD_WEIGHTS="-3,1")
    host_case(knobs, {"shard_weights": ""}, SHARD_WEIGHTS="")


# ---- the pool table: which devices, how many contexts of each

def test_pool_devices(knobs):
    """The parser names the devices as the text does; an index that is not there (DEVICES=1,1,7; DEVICE=9) is the
    pool's to drop when it sets itself up, not the parser's."""
    def devices(visible=4, **env):
        return knobs("pool", visible, **env)["devices"]
    assert devices() == "0"
    assert devices(DEVICES="all") == "0,1,2,3"
    assert devices(DEVICES="2") == "0,1"
    assert devices(DEVICES="0") == "0"              # no count: device 0
    assert devices(DEVICES="9") == "0,1,2,3"
    assert devices(DEVICES="1,1,3") == "1,1,3"
    assert devices(DEVICES="1,1,7") == "1,1,7"      # kept by the parser
    assert devices(DEVICE="2") == "2"
    assert devices(DEVICE="9") == "9"               # kept by the parser
    assert devices(LOCAL_RANK="5") == "1"
    assert devices(visible=1, LOCAL_RANK="5") == "0"
    assert devices(DEVICES="3", DEVICE="2", LOCAL_RANK="1") == "0,1,2"     # DEVICES wins
    assert devices(DEVICE="2", LOCAL_RANK="1") == "2"                      # then DEVICE
    assert devices(DEVICES="all", visible=0) == ""


def test_pool_lanes(knobs):
    """LANES is at least 1, SMALL_LANES at least LANES."""
    def lanes(**env):
        k = knobs("pool", 4, **env)
        return k["lanes"], k["small_lanes"]
    assert lanes() == ("3", "16")
    assert lanes(LANES="0") == ("1", "16")
    assert lanes(LANES="-1") == ("1", "16")
    assert lanes(LANES="5") == ("5", "16")
    assert lanes(LANES="20") == ("20", "20")
    assert lanes(SMALL_LANES="1") == ("3", "3")
    assert lanes(SMALL_LANES="8") == ("3", "8")
    assert lanes(LANES="2", SMALL_LANES="0") == ("2", "2")


def test_every_switch_is_documented():
    """The "ZOPFLI_AMD_..." string literals of the sources == the names in INTEGRATION.md (ZOPFLI_AMD_LIB, which the
    Python side reads, is in the table)."""
    name = re.compile(r'"(ZOPFLI(?:PNG)?_AMD_[A-Z0-9_]+)"')
    read = set()
    files = glob.glob(os.path.join(ROOT, "zopfli_amd", "*.py"))
    for base, _, names in os.walk(os.path.join(ROOT, "zopfli_amd", "csrc")):
        files += [os.path.join(base, n) for n in names if n.endswith((".h", ".cc", ".hip", ".c", ".py"))]
    for path in files:
        with open(path, errors="replace") as f:
            read |= set(name.findall(f.read()))
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        documented = set(re.findall(r"ZOPFLI(?:PNG)?_AMD_[A-Z0-9_]+", f.read()))
    assert len(read) > 40
    assert read == documented, (sorted(read - documented), sorted(documented - read))
