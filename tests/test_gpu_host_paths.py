"""The paths of the host layer (csrc/host/deflate.cc: the phases of DeflateParts; api.cc: the dealing) on the product
library and a real device: every one gives the reference's stream.  The input is the mix on which each phase has work
— three master blocks, the first split finds points, the second split is tried, fixed-tree re-parses are requested
(six; none wins), and dynamic and stored blocks are written; its SHA-256 comes from the reference on the CPU
(tests/golden/host_paths.json, written by tests/golden/make_golden.py --host-paths).  Every path runs in a fresh
process: the switches are read once per process."""
import json
import os
import subprocess
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

PATHS = {
    "default": {},
    "device_split_forced": {"DEVICE_SPLIT": "2", "DEVICE_SPLIT_FROM": "1"},
    "host_split": {"DEVICE_SPLIT": "0"},
    "host_bit_writer": {"DEVICE_ENCODE": "0"},
    "dealt_over_contexts": {"SPLIT_MB": "2", "DEAL_AFTER": "0"},
    "split_one_by_one": {"BATCH_SPLIT": "0"},
    "a_part_per_batch": {"PARTS_PER_BATCH": "1"},
}

CHILD = (
    "import hashlib, sys\n"
    "sys.path.insert(0, %r)\n"
    "from zopfli_amd import ZopfliOptions, api, generate\n"
    "case = %r\n"
    "data = b''.join(generate(i['cls'], i['size']) for i in case['input'])\n"
    "opt = ZopfliOptions(case['numiterations'], case['blocksplitting'], case['blocksplittingmax'], 1, 0)\n"
    "out = api.compress(data, case['format'], opt)\n"
    "print(len(out), hashlib.sha256(out).hexdigest())\n")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(TESTS, "golden", "host_paths.json")) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_host_path_gives_the_reference_stream(gpu_lib, golden, path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZOPFLI_AMD_") or k == "ZOPFLI_AMD_LIB"}
    env.update({"ZOPFLI_AMD_" + k: v for k, v in PATHS[path].items()})
    case = {k: golden[k] for k in ("input", "format", "numiterations", "blocksplitting", "blocksplittingmax")}
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, case)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    size, digest = r.stdout.split()[-2:]
    assert (int(size), digest) == (golden["outsize"], golden["sha256"])
    assert r.stderr.count("block split points") >= 3          # (verbose: the reference's lines, a part at a time)
