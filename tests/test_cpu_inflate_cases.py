"""The rules of device/zmx_inflate.h on the CPU, through tests/hostlib/inflate_print.cc, which runs the kernel's own walk
with the 64 lanes one after the other — built plain and with sanitizers.  inflate_cases.py's reference decoder is held
against zlib's own inflate first (the bytes and unused_data on every valid stream, accept or reject on every malformed
one), then both programs against the reference on every case, statuses included, and the addresses they touched against
the ranges.  Every planted case must reach what its name says."""
import functools
import os
import subprocess
import zlib

import pytest

import inflate_cases as ic
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    if request.param == "plain":
        subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "inflate.mk"])
        return os.path.join(BUILD, "inflate_print")
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "inflate.mk", "SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san"])
    return os.path.join(BUILD, "inflate_print_san")


@functools.lru_cache(maxsize=None)
def reference(case):
    return ic.inflate_ref(case.fmt, case.stream)


def run(exe, jobs):
    """jobs: (fmt, stream, capacity or None, in_shift, out_shift) -> the program's lines as lists of fields"""
    text = "".join(f"{fmt} {'null' if cap is None else cap} {si} {so} {stream.hex() or '-'}\n" for fmt, stream, cap, si, so in jobs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = [line.split() for line in r.stdout.splitlines()]
    assert len(lines) == len(jobs)
    return lines


def check_line(case, fields, ref, cap, stored_out):
    """the program's line against the reference; the addresses inside the ranges"""
    want_status = ref["kernel_status"]
    if want_status == ic.OK and cap is not None and ref["outsize"] > cap:
        want_status = ic.CAPACITY
    got = [int(v) for v in fields[:7]]
    assert got[:6] == [want_status, ref["outsize"], ref["consumed"], ref["block"], ref["stored_check"], ref["stored_isize"]], case
    assert got[6] == zlib.crc32(stored_out) & 0xffffffff, case
    read_lo, read_hi, write_lo, write_hi = fields[7:11]
    if read_lo != "-":
        assert 0 <= int(read_lo) and int(read_hi) <= len(case.stream), case
        # (all that was consumed was read, and on a valid stream nothing behind the trailer had to be)
        assert int(read_lo) == 0 and int(read_hi) >= ref["consumed"], case
    else:
        assert ref["consumed"] == 0 or len(case.stream) == 0, case
    if write_lo != "-":
        assert cap is not None and 0 <= int(write_lo) and int(write_hi) <= cap, case
        assert (int(write_lo), int(write_hi)) == (0, len(stored_out)), case
    else:
        assert len(stored_out) == 0, case


def test_constants_are_the_headers(exe):
    r = subprocess.run([exe, "constants"], capture_output=True, text=True)
    ring, stretch, lit_root, dist_root, scratch = (int(v) for v in r.stdout.split())
    assert (ring, stretch, lit_root, dist_root) == (ic.RING, ic.STRETCH, ic.LIT_ROOT, ic.DIST_ROOT)
    assert ring >= 32768 + stretch + 2 * 258 and scratch <= 65536      # the window holds 32 KiB behind what waits for its flush; two waves a CU


def test_reference_equals_zlib_on_valid_streams():
    for case in ic.valid_cases():
        ref = reference(case)
        accepted, out, consumed = ic.zlib_verdict(case.fmt, case.stream)
        assert accepted, case
        assert ref["status"] == ic.OK, (case, ic.STATUS_NAMES[ref["status"]])
        assert ref["out"] == out == case.expect, case
        assert ref["consumed"] == consumed, case


def test_reference_agrees_with_zlib_on_malformed_streams():
    for case in ic.malformed_cases() + ic.trailer_cases():
        ref = reference(case)
        assert ref["status"] == case.status, (case, ic.STATUS_NAMES[ref["status"]])
        assert not ic.zlib_verdict(case.fmt, case.stream)[0], case
    assert {c.status for c in ic.malformed_cases() + ic.trailer_cases()} == set(range(1, 17)) - {ic.CAPACITY}


def test_cases_reach_what_their_names_say():
    seen_kinds, formats = set(), set()
    for case in ic.valid_cases():
        trace = reference(case)["trace"]
        seen_kinds |= set(trace["kinds"])
        formats.add(case.fmt)
        for key, want in case.wants.items():
            if key == "crossed":
                assert want <= trace["crossed"], (case, trace["crossed"])
            else:
                assert trace[key] == want, (case, key, trace[key])
    assert seen_kinds == {0, 1, 2} and formats == {ic.GZIP, ic.ZLIB, ic.DEFLATE}
    by_name = {c.name: c for c in ic.valid_cases()}
    # zlib's own streams: level 0 is stored, Z_FIXED fixed, the others dynamic where there is something to gain
    for name, case in by_name.items():
        kinds = set(reference(case)["trace"]["kinds"])
        if name.startswith("zlib_text_200000_l0"):
            assert kinds == {0} and len(reference(case)["trace"]["kinds"]) >= 4      # several stored blocks of 65 535 bytes
        if name.startswith("zlib_text_200000_l6_fixed"):
            assert kinds == {1}
        if name.startswith("zlib_text_200000_l9"):
            assert kinds == {2} and reference(case)["trace"]["longest"] > ic.LIT_ROOT   # codes beyond the primary table
        if name.startswith(("zlib_text_200000_l6_default", "zlib_text_200000_l9", "zlib_text_200000_l6_fixed")):
            assert reference(case)["trace"]["wrap"] and reference(case)["trace"]["seam"]    # matches over the ring's wrap and over a flush
    assert 15 in (reference(c)["trace"]["longest"] for c in ic.planted_cases())
    # the stretch sizes: one below to two above, and two stretches plus one
    sizes = {len(c.expect) for c in ic.planted_cases() if c.name.startswith("output_of_")}
    assert sizes == {ic.STRETCH + d for d in (-2, -1, 0, 1, 2)} | {2 * ic.STRETCH + 1}
    assert sorted(c.wants["stored_at"][0] for c in ic.planted_cases() if c.name.startswith("stored_at_bit_")) == list(range(8))
    cuts = [c for c in ic.malformed_cases() if "_cut_" in c.name]
    assert len(cuts) == 80 and all(c.status == ic.TRUNCATED for c in cuts)


def test_programs_equal_the_reference_on_valid_streams(exe):
    cases = ic.valid_cases()
    shifts = [(0, 0), (1, 1), (3, 7), (15, 15)]
    jobs = [(c.fmt, c.stream, len(c.expect), *shifts[i % 4]) for i, c in enumerate(cases)]
    for case, fields in zip(cases, run(exe, jobs)):
        check_line(case, fields, reference(case), len(case.expect), case.expect)


def test_programs_equal_the_reference_on_malformed_streams(exe):
    cases = ic.malformed_cases() + ic.trailer_cases()
    jobs = [(c.fmt, c.stream, 4096, i % 16, (5 * i) % 16) for i, c in enumerate(cases)]
    for case, fields in zip(cases, run(exe, jobs)):
        ref = reference(case)
        check_line(case, fields, ref, 4096, ref["out"][:4096])


def test_size_only_and_short_capacities(exe):
    """The size-only mode writes nothing and gives the same outsize; with a capacity below the size — one byte short, half, none
    — the walk goes on, stores nothing at or beyond it and reports CAPACITY with the size."""
    cases = [c for c in ic.planted_cases()] + [c for c in ic.zlib_cases() if "_257_" in c.name or "_65536_l6_default" in c.name]
    jobs, what = [], []
    for i, case in enumerate(cases):
        n = len(case.expect)
        for cap in [None] + ([n - 1, n // 2, 0] if n else []):
            jobs.append((case.fmt, case.stream, cap, i % 16, (3 * i) % 16))
            what.append((case, cap))
    for (case, cap), fields in zip(what, run(exe, jobs)):
        check_line(case, fields, reference(case), cap, b"" if cap is None else case.expect[:cap])
        assert int(fields[0]) == (ic.OK if cap is None else ic.CAPACITY), case
