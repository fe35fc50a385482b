"""The device layer's switches (zopfli_amd/csrc/device/zmx_knobs.h): tests/hostlib/knob_print.cc parses this
process's environment with the header's own function and prints the struct; the defaults and the odd inputs of every
switch whose text is not taken as it stands.  Also: every ZOPFLI_AMD_* / ZOPFLIPNG_AMD_* name the sources read is in
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

    def run(**env):
        """The parsed struct as {field: text} with only ZOPFLI_AMD_<KEY>=value of `env` set."""
        clean = {k: v for k, v in os.environ.items() if not k.startswith("ZOPFLI_AMD_")}
        clean.update({"ZOPFLI_AMD_" + k: str(v) for k, v in env.items()})
        out = subprocess.run([KNOB_PRINT], env=clean, capture_output=True, text=True, check=True).stdout
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
