"""Input that already lives in device memory: zmx_compress_device, zmx_set_input_device, zmx_master_block_costs_device and
zmx_last_input_traffic against the host-pointer calls on the same bytes.  Device buffers come from torch."""
import ctypes
import hashlib
import json
import os
import threading

import numpy as np
import pytest
import torch

import device_input_cases as cases
from zopfli_amd import Context, ZopfliOptions, api, generate

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "vectors.json")
ZMX_ERR_REFUSED = 3


def _dev(data):
    """The bytes as a uint8 tensor in device memory (an empty input: an empty tensor)."""
    if len(data) == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


_inputs = {}


def _input(name):
    if name not in _inputs:
        if name == "one":
            data = b"a"
        elif name == "T70000":
            data = generate("T", 70000)
        elif name == "M1200000":
            data = generate("M", 1200000)
        elif name == "random100000":
            data = np.random.default_rng(1).integers(0, 256, 100000, dtype=np.uint8).tobytes()
        elif name == "Z300000":
            data = generate("Z", 300000)
        elif name == "text+zeros":
            data = generate("T", 50000) + bytes(20000)
        else:
            raise KeyError(name)
        _inputs[name] = data
    return _inputs[name]


PARITY_INPUTS = ["one", "T70000", "M1200000", "random100000", "Z300000", "text+zeros"]


@pytest.mark.parametrize("splitting", [0, 1])
@pytest.mark.parametrize("fmt", [api.FORMAT_GZIP, api.FORMAT_ZLIB, api.FORMAT_DEFLATE])
@pytest.mark.parametrize("name", PARITY_INPUTS)
def test_parity_with_host_call(gpu_lib, name, fmt, splitting):
    data = _input(name)
    opt = ZopfliOptions(5, splitting)
    want = api.compress(data, fmt, opt, lib=gpu_lib)
    assert api.compress_device(_dev(data), fmt=fmt, options=opt, lib=gpu_lib) == want


@pytest.mark.parametrize("splitting", [0, 1])
@pytest.mark.parametrize("fmt", [api.FORMAT_GZIP, api.FORMAT_ZLIB, api.FORMAT_DEFLATE])
def test_parity_empty_input(gpu_lib, fmt, splitting):
    """No bytes: a null pointer, a pointer into device memory, an empty tensor."""
    opt = ZopfliOptions(5, splitting)
    want = api.compress(b"", fmt, opt, lib=gpu_lib)
    some = _dev(b"0123456789abcdef")
    assert api.compress_device(0, 0, fmt, opt, lib=gpu_lib) == want
    assert api.compress_device(some.data_ptr(), 0, fmt, opt, lib=gpu_lib) == want
    assert api.compress_device(_dev(b""), fmt=fmt, options=opt, lib=gpu_lib) == want


def _golden():
    with open(GOLDEN) as f:
        return [c for c in json.load(f) if c["insize"] <= 1200000]


def _gid(c):
    return (f"{c['input'].get('name', c['input'].get('cls'))}-{c['insize']}-f{c['format']}-n{c['numiterations']}"
            f"-s{c['blocksplitting']}")


@pytest.mark.parametrize("case", _golden(), ids=_gid)
def test_golden(gpu_lib, case):
    """The reference's bytes (SHA-256 of its output, tests/golden/vectors.json) from a device buffer."""
    spec = case["input"]
    if spec["kind"] == "literal":
        from golden.make_golden import LITERALS
        data = LITERALS[spec["name"]]
    else:
        data = generate(spec["cls"], spec["size"], spec.get("seed"))
    opt = ZopfliOptions(case["numiterations"], case["blocksplitting"], case["blocksplittingmax"])
    out = api.compress_device(_dev(data), fmt=case["format"], options=opt, lib=gpu_lib)
    assert len(out) == case["outsize"]
    assert hashlib.sha256(out).hexdigest() == case["sha256"]


@pytest.mark.parametrize("offset", [1, 3, 7])
def test_unaligned_views(gpu_lib, offset):
    """The input starts 1, 3, 7 bytes into an allocation, 64 guard bytes of 0xA5 on both sides: the same stream as
    from an aligned buffer, and nothing of the allocation changes."""
    data = _input("T70000")
    opt = ZopfliOptions(5)
    want = api.compress_device(_dev(data), options=opt, lib=gpu_lib)
    whole = torch.full((64 + offset + len(data) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    view = whole[64 + offset:64 + offset + len(data)]
    view.copy_(_dev(data))
    before = whole.cpu().numpy().copy()
    assert view.data_ptr() % 8 == (whole.data_ptr() + 64 + offset) % 8 and view.data_ptr() % 2 == 1
    assert api.compress_device(view, options=opt, lib=gpu_lib) == want
    after = whole.cpu().numpy()
    assert np.array_equal(before, after)
    assert np.all(after[:64 + offset] == 0xA5) and np.all(after[-64:] == 0xA5)


def test_non_contiguous_tensor_is_refused(gpu_lib):
    t = _dev(_input("T70000"))[::2]
    with pytest.raises(ValueError):
        api.compress_device(t, lib=gpu_lib)


def _host_costs(lib, data):
    fn = lib.zmx_master_block_costs
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double), ctypes.c_size_t]
    fn.restype = ctypes.c_int
    cost = np.zeros(max(1, (len(data) + 999999) // 1000000), dtype=np.float64)
    n = fn(data, len(data), cost.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cost.size)
    assert n == cost.size
    return cost


def test_master_block_costs_device(gpu_lib):
    """k_probe_counts against the host's probes, double for double: the last probe against the end of the input,
    probes at a master-block seam, a mixed input of 2 000 064 bytes; after zmx_set_input as after
    zmx_set_input_device."""
    mixed = cases.mixed(2000064)
    crafted, _ = cases.crafted_probes()
    ctx = Context(0, gpu_lib)
    try:
        inputs = [mixed[:n] for n in cases.SEAM_SIZES] + [crafted, cases.runs_threshold(2)]
        interesting = False
        for data in inputs:
            want = _host_costs(gpu_lib, data)
            t = _dev(data)
            ctx.set_input_device(t.data_ptr(), len(data))
            got = ctx.master_block_costs_device()
            assert got.tobytes() == want.tobytes(), (len(data), got, want)
            plain = [(min(len(data), (b + 1) * 1000000) - b * 1000000) / 1e6 for b in range(len(want))]
            interesting |= bool(np.any(want != np.array(plain)))
        assert interesting, "no probe found a run or a few-valued stretch: the inputs test nothing"
        ctx.set_input(mixed)
        assert ctx.master_block_costs_device().tobytes() == _host_costs(gpu_lib, mixed).tobytes()
    finally:
        ctx.close()


def _positions_matched(lib):
    m = (ctypes.c_double * 4)()
    lib.zmx_last_match_timing(m)
    return m[3]


@pytest.mark.parametrize("run", cases.TAIL_RUNS + [None], ids=lambda r: f"run{r}")
def test_table_reuse_from_device_input(gpu_lib, run):
    """Child tables built from a parent's (zmx_tables_build_from) on an input set from device memory: the same match
    records as on a host-set input, and as many positions matched again — the reuse is taken, by the same plan
    (k_tail_runs gives what the host's walk over its own copy gives)."""
    data, blocks, want = cases.tail_case(generate("T", cases.TAIL_PARENT), run)
    assert cases.tail_run_start(data, *blocks[-2]) == want
    result = []
    for on_device in (False, True):
        ctx = Context(0, gpu_lib)
        try:
            if on_device:
                t = _dev(data)
                ctx.set_input_device(t.data_ptr(), len(data))
                t.zero_()     # (the context has its own copy)
                torch.cuda.synchronize()
            else:
                ctx.set_input(data)
            parent = ctx.build_tables([(0, cases.TAIL_PARENT)], matches_only=True)
            before = _positions_matched(gpu_lib)
            child = ctx.build_tables(blocks, parent=parent, matches_only=False)
            matched = _positions_matched(gpu_lib) - before
            result.append((child.match_digest(), matched))
            child.free()
            parent.free()
        finally:
            ctx.close()
    print("positions matched again (host input, device input):", result[0][1], result[1][1])
    assert result[1][0] == result[0][0]
    assert result[1][1] == result[0][1]
    assert result[1][1] < cases.TAIL_PARENT, "every position was matched again: the parent's records were not reused"


@pytest.mark.parametrize("kind", ["random", "text"])
def test_deflate_range_on_device_input(gpu_lib, kind):
    """zmx_deflate_range on an input set from device memory: its blob — stored blocks with their bytes — merges to
    ZopfliDeflate of the bytes."""
    data = (np.random.default_rng(2).integers(0, 256, 150000, dtype=np.uint8).tobytes() if kind == "random"
            else generate("T", 150000))
    opt = ZopfliOptions(5)
    want, _ = api.deflate(data, options=opt, lib=gpu_lib)
    ctx = Context(0, gpu_lib)
    try:
        t = _dev(data)
        ctx.set_input_device(t.data_ptr(), len(data))
        blob = ctx.deflate_range(opt, 0, len(data))
        assert ctx.merge([blob]) == want
        traffic = api.last_input_traffic(gpu_lib)
        if kind == "random":
            assert 0 < traffic[2] <= len(data)
        else:
            assert traffic[2] == 0
    finally:
        ctx.close()


def test_input_traffic(gpu_lib):
    """What crosses the bus, as conditions: nothing of a text input, the stored blocks' bytes of a random one; a host
    call uploads all of its input."""
    opt = ZopfliOptions(5)
    for name in ("T70000", "text+zeros"):
        data = _input(name)
        api.compress_device(_dev(data), options=opt, lib=gpu_lib)
        t = api.last_input_traffic(gpu_lib)
        assert t[0] == 0 and t[2] == 0 and t[1] >= len(data), (name, t)
        api.compress(data, options=opt, lib=gpu_lib)
        t = api.last_input_traffic(gpu_lib)
        assert t[0] >= len(data) and t[1] == 0 and t[2] == 0, (name, t)
    data = _input("random100000")
    api.compress_device(_dev(data), options=opt, lib=gpu_lib)
    t = api.last_input_traffic(gpu_lib)
    assert t[0] == 0 and 0 < t[2] <= len(data), t


def _raw_call(lib, ptr, size):
    """zmx_compress_device with an output array of its own: (return code, out pointer after, outsize after, pointer
    before)."""
    fn = lib.zmx_compress_device
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    libc = ctypes.CDLL(None)
    libc.malloc.restype = ctypes.c_void_p
    libc.malloc.argtypes = [ctypes.c_size_t]
    libc.free.argtypes = [ctypes.c_void_p]
    addr = libc.malloc(16)
    ctypes.memmove(addr, b"0123456789abcdef", 16)
    out, outsize = ctypes.c_void_p(addr), ctypes.c_size_t(3)
    opt = ZopfliOptions(5)
    rc = fn(ctypes.byref(opt), api.FORMAT_GZIP, ptr, size, ctypes.byref(out), ctypes.byref(outsize))
    kept = ctypes.string_at(out.value, 16) if out.value == addr else None
    result = (rc, out.value, outsize.value, addr, kept)
    libc.free(out.value)
    return result


def test_refusals(gpu_lib):
    """A host pointer and a null pointer with a size are refused on the host (ZMX_ERR_REFUSED), the output array stays
    as it was, and the thread's next valid call succeeds."""
    host = np.frombuffer(_input("T70000"), dtype=np.uint8).copy()
    for ptr, size in ((host.ctypes.data, host.size), (0, 5)):
        rc, out, outsize, addr, kept = _raw_call(gpu_lib, ptr, size)
        assert rc == -1
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, gpu_lib.zmx_last_error()
        assert (out, outsize, kept) == (addr, 3, b"0123456789abcdef")
        with pytest.raises(RuntimeError):
            api.compress_device(ptr, size, lib=gpu_lib)
        ctx = Context(0, gpu_lib)
        try:
            with pytest.raises(RuntimeError):
                ctx.set_input_device(ptr, size)
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
        finally:
            ctx.close()
        data = _input("T70000")
        opt = ZopfliOptions(5)
        assert api.compress_device(_dev(data), options=opt, lib=gpu_lib) == api.compress(data, options=opt, lib=gpu_lib)
    # a range that leaves its allocation
    t = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        api.compress_device(t.data_ptr(), 1 << 40, lib=gpu_lib)
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED


def test_concurrent_callers(gpu_lib):
    """Four threads, four device tensors of 64 KiB to 300 KB, two rounds each: every output is the host call's."""
    opt = ZopfliOptions(5)
    datas = [generate("T", 65536), generate("X", 150000), generate("M", 300000), generate("P", 200000)]
    want = [api.compress(d, options=opt, lib=gpu_lib) for d in datas]
    tensors = [_dev(d) for d in datas]
    torch.cuda.synchronize()
    got = [[None, None] for _ in datas]
    errors = []

    def work(i):
        try:
            for r in range(2):
                got[i][r] = api.compress_device(tensors[i], options=opt, lib=gpu_lib)
        except Exception as e:   # noqa: BLE001 (reported below, on the test's thread)
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(datas))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(len(datas)):
        assert got[i][0] == want[i] and got[i][1] == want[i], i


def test_buffer_may_be_reused_after_the_call(gpu_lib):
    """Nothing reads the caller's buffer once the call has returned: zeroed right after, the output is still the
    reference's."""
    data = _input("M1200000")
    opt = ZopfliOptions(5)
    t = _dev(data)
    out = api.compress_device(t, options=opt, lib=gpu_lib)
    t.zero_()
    torch.cuda.synchronize()
    assert out == api.compress(data, options=opt, lib=gpu_lib)
