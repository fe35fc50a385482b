"""The match record (zopfli_amd/csrc/device/zmx_record.h: recs[] and pool[]) on the CPU: tests/hostlib/record_print.cc
packs a table of records the two ways the match kernels do, requires the same eight words of both, and decodes them
with every reader the header offers.  Its output is held against the few lines below, a model of the header's layout
comment: the words, the header fields, the change points in order, and sublen[3 .. 258] by each reader."""
import os
import struct
import subprocess

from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
LENGTHS = range(3, 259)


def rec(length, dist, same, literal, cps, front=0, back=0):
    return dict(length=length, dist=dist, same=same, literal=literal, cps=list(cps), front=front, back=back)


def held(cps, same, literal, front=0, back=0):
    """A record whose length and distance are its last change point's, as the match kernels leave it."""
    return rec(cps[-1][0], cps[-1][1], same, literal, cps, front, back)


def ramp(n, first=3, step=1, dist0=1, dstep=37):
    """n change points of ascending length; the distances stay inside the window."""
    return [(first + step * i, (dist0 + dstep * i - 1) % 32768 + 1) for i in range(n)]


def cases():
    out = []
    # no change point: the short forms (rec[0] = 0 / 1) and a length-2 result
    out += [rec(0, 0, 0, 0, []), rec(1, 0, 65535, 255, []), rec(2, 7, 1, 65, [])]
    # every inline count, the record's length its last change point's; then the pool
    for n in range(1, 9):
        out.append(held(ramp(n, first=3 + n, step=9), n, 16 * n))
    out.append(held(ramp(9), 2, 97, front=3, back=5))
    out.append(held([(3 + i, 32768 - 7 * i) for i in range(256)], 65535, 255, front=1, back=2))
    out.append(held(ramp(10, first=4, step=4), 0, 0))   # the pool's last record: nothing in front of it or behind it
    # the edges of every field
    for dist in (1, 255, 256, 32768):
        out.append(rec(3, dist, 0, 0, [(3, dist)]))
        out.append(rec(258, dist, 65535, 255, [(258, dist)]))
        out.append(rec(258, dist, 0, 255, [(3, 1), (130, 255), (131, 256), (257, 32768), (258, dist)]))
    out.append(held([(3 + 36 * i, d) for i, d in enumerate((32768, 1, 255, 256, 32768, 1, 255))] + [(258, 256)], 65535, 0))
    # fewer than 8 change points, the last of length 258: its threshold byte is the padding's 255
    out.append(rec(258, 5, 300, 32, [(3, 2), (100, 3), (258, 5)]))
    out.append(rec(258, 1, 258, 0, [(258, 1)]))
    out.append(rec(258, 77, 4, 1, ramp(6, first=10, step=20) + [(258, 77)]))
    # eight change points that end below 258: lengths above the last one are not held
    out.append(held(ramp(7, first=5, step=11) + [(99, 1234)], 9, 200))
    return out


CASES = cases()


# ---- the model: zmx_record.h's layout comment
def model_words(r, pool_off):
    n = len(r["cps"])
    inline = bytearray(24)
    for e, (ln, d) in enumerate(r["cps"][:8]):
        inline[3 * e:3 * e + 3] = bytes((ln - 3, d & 255, d >> 8))
    w = [r["length"] | r["dist"] << 16, r["same"] | r["literal"] << 16 | (n if n <= 8 else 0xFF) << 24]
    w += struct.unpack("<6I", bytes(inline))
    if n > 8:
        w[2], w[3] = pool_off, n
    return w


def model_sublen(cps):
    """sublen[len] = the distance of the first change point with a length >= len; 0: not held."""
    return [next((d for ln, d in cps if ln >= length), 0) for length in LENGTHS]


def model_thresholds(cps):
    """k_codes' search: the first of eight thresholds (len - 3; 255 from the record's count on) >= len - 3, or the last
    field; a field behind the record's count is zero."""
    thr = [ln - 3 for ln, _ in cps] + [255] * (8 - len(cps))
    dist = [d for _, d in cps] + [0] * (8 - len(cps))
    return [dist[next((e for e in range(8) if thr[e] >= length - 3), 7)] for length in LENGTHS]


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "record.mk", *extra])


def _run(exe, tmp_path):
    table = os.path.join(str(tmp_path), "records.txt")
    with open(table, "w") as f:
        for r in CASES:
            cps = " ".join(f"{ln} {d}" for ln, d in r["cps"])
            f.write(f'{r["front"]} {r["back"]} {r["length"]} {r["dist"]} {r["same"]} {r["literal"]} {len(r["cps"])} {cps}\n')
    p = subprocess.run([exe, table], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert lines[-1] == f"ok {len(CASES)}"
    assert len(lines) == 8 * len(CASES) + 1
    return [dict(ln.split(" ", 1) if " " in ln else (ln, "") for ln in lines[8 * i:8 * i + 8]) for i in range(len(CASES))]


def _check(got):
    pool_at = 0
    for i, (r, g) in enumerate(zip(CASES, got)):
        n = len(r["cps"])
        off = 0
        if n > 8:
            off = pool_at + r["front"]
            pool_at = off + n + r["back"]
        assert [int(x, 16) for x in g["rec"].split()] == model_words(r, off), i
        assert [int(x) for x in g["hdr"].split()] == [r["length"], r["dist"], r["same"], r["literal"], n if n <= 8 else 255,
                                                      int(n > 8), off if n > 8 else 0, n if n > 8 else 0], i
        assert g["cps"].split() == [f"{ln}:{d}" for ln, d in r["cps"]], i
        want = model_sublen(r["cps"])
        assert [int(x) for x in g["walk"].split()] == want, i
        if n <= 8:
            assert [int(x) for x in g["scan"].split()] == want, i
            assert [int(x) for x in g["acc"].split()] == want, i
            assert [int(x) for x in g["thr"].split()] == model_thresholds(r["cps"]), i
            assert g["pool"] == "-", i
        else:
            assert [int(x) for x in g["pool"].split()] == want, i
            assert g["scan"] == g["acc"] == g["thr"] == "-", i


def test_cases_cover_the_format():
    """What the table has to hold (the model's own arithmetic, no program)."""
    counts = {len(r["cps"]) for r in CASES}
    assert set(range(9)) <= counts and 9 in counts and 256 in counts
    cps = [cp for r in CASES for cp in r["cps"]]
    assert {3, 258} <= {ln for ln, _ in cps} and {1, 255, 256, 32768} <= {d for _, d in cps}
    assert {0, 65535} <= {r["same"] for r in CASES} and {0, 255} <= {r["literal"] for r in CASES}
    assert any(len(r["cps"]) < 8 and r["cps"] and r["cps"][-1][0] == 258 for r in CASES)
    assert any(len(r["cps"]) > 8 and r["front"] and r["back"] for r in CASES)
    for r in CASES:
        lens = [ln for ln, _ in r["cps"]]
        assert lens == sorted(set(lens)) and all(3 <= ln <= 258 for ln in lens)
        assert all(1 <= d <= 32768 for _, d in r["cps"])
        if r["cps"]:
            assert (r["length"], r["dist"]) == r["cps"][-1]
    # the threshold search agrees with sublen for every length the record holds (and beyond, unless the record is full)
    for r in CASES:
        if len(r["cps"]) <= 8:
            last = r["cps"][-1][0] if r["cps"] else 2
            assert model_thresholds(r["cps"])[:last - 2] == model_sublen(r["cps"])[:last - 2]


def test_record_format(tmp_path):
    _make()
    _check(_run(os.path.join(BUILD, "record_print"), tmp_path))


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): an overflow record is also decoded
    from a heap array that ends with its last pool entry, so a read behind the record's count is reported."""
    _make("SANITIZE=-fsanitize=address,undefined", "OUT_NAME=record_print_san")
    _check(_run(os.path.join(BUILD, "record_print_san"), tmp_path))
