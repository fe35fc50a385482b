"""ctypes mirror of include/zopfli_amd.h (reference names and argument meaning)."""
import ctypes
import os

from ._build import LIB

# (a variant build for A/B measurements: tools/build_variant.py)
if os.environ.get("ZOPFLI_AMD_LIB"):
    LIB = os.environ["ZOPFLI_AMD_LIB"]

FORMAT_GZIP, FORMAT_ZLIB, FORMAT_DEFLATE = 0, 1, 2  # zopfli.h:70-74
CRC32, ADLER32 = 0, 1  # ZMX_CRC32, ZMX_ADLER32
ZMX_HIST = 320


class ZopfliOptions(ctypes.Structure):
    """zopfli.h:33-64; defaults as ZopfliInitOptions (util.c:28)."""
    _fields_ = [("verbose", ctypes.c_int), ("verbose_more", ctypes.c_int), ("numiterations", ctypes.c_int),
                ("blocksplitting", ctypes.c_int), ("blocksplittinglast", ctypes.c_int),
                ("blocksplittingmax", ctypes.c_int)]

    def __init__(self, numiterations=15, blocksplitting=1, blocksplittingmax=15, verbose=0, verbose_more=0):
        super().__init__(verbose, verbose_more, numiterations, blocksplitting, 0, blocksplittingmax)


class ZmxBlock(ctypes.Structure):
    _fields_ = [("instart", ctypes.c_uint64), ("inend", ctypes.c_uint64)]


_lib = None
_libc = ctypes.CDLL(None)
_libc.free.argtypes = [ctypes.c_void_p]
_libc.malloc.argtypes = [ctypes.c_size_t]
_libc.malloc.restype = ctypes.c_void_p
_libc.realloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
_libc.realloc.restype = ctypes.c_void_p
_u8p = ctypes.POINTER(ctypes.c_ubyte)


def _pow2ceil(n):
    cap = 1
    while cap < n:
        cap <<= 1
    return cap


def _owned_array(addr, size):
    """A numpy uint8 view of a malloc'ed buffer that frees it when the array is collected."""
    import weakref

    import numpy as np
    if size == 0:
        _libc.free(addr)
        return np.zeros(0, dtype=np.uint8)
    buf = (ctypes.c_ubyte * size).from_address(addr)
    weakref.finalize(buf, _libc.free, addr)
    return np.frombuffer(buf, dtype=np.uint8)


def bind(lib):
    """Declares the prototypes of include/zopfli_amd.h on a loaded library."""
    P, sz, vp = ctypes.POINTER, ctypes.c_size_t, ctypes.c_void_p
    opt = P(ZopfliOptions)
    lib.ZopfliInitOptions.argtypes = [opt]
    lib.ZopfliInitOptions.restype = None
    lib.ZopfliCompress.argtypes = [opt, ctypes.c_int, ctypes.c_char_p, sz, P(_u8p), P(sz)]
    lib.ZopfliCompress.restype = None
    for name in ("ZopfliGzipCompress", "ZopfliZlibCompress"):
        f = getattr(lib, name)
        f.argtypes = [opt, ctypes.c_char_p, sz, P(_u8p), P(sz)]
        f.restype = None
    lib.ZopfliDeflate.argtypes = [opt, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, P(ctypes.c_ubyte), P(_u8p),
                                  P(sz)]
    lib.ZopfliDeflate.restype = None
    lib.ZopfliDeflatePart.argtypes = [opt, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, sz, P(ctypes.c_ubyte),
                                      P(_u8p), P(sz)]
    lib.ZopfliDeflatePart.restype = None
    lib.zmx_device_count.restype = ctypes.c_int
    lib.zmx_last_error.restype = ctypes.c_char_p
    lib.zmx_last_error_class.restype = ctypes.c_int
    lib.zmx_host_cache_trim.restype = ctypes.c_size_t
    lib.zmx_ctx_create.argtypes = [ctypes.c_int, P(vp)]
    lib.zmx_ctx_destroy.argtypes = [vp]
    lib.zmx_ctx_destroy.restype = None
    lib.zmx_set_input.argtypes = [vp, ctypes.c_char_p, sz]
    lib.zmx_tables_build.argtypes = [vp, P(ZmxBlock), sz, P(vp)]
    lib.zmx_tables_build_matches.argtypes = [vp, P(ZmxBlock), sz, P(vp)]
    lib.zmx_tables_build_from.argtypes = [vp, vp, P(ZmxBlock), sz, P(vp)]
    lib.zmx_tables_free.argtypes = [vp, vp]
    lib.zmx_tables_trim.argtypes = [vp, vp]
    lib.zmx_tables_free.restype = None
    lib.zmx_lz77_greedy.argtypes = [vp, vp, ctypes.c_int, P(ctypes.c_uint32), P(ctypes.c_uint32)]
    lib.zmx_squeeze_run.argtypes = [vp, vp, P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_int32),
                                    P(ctypes.c_uint32), P(ctypes.c_uint32)]
    lib.zmx_store_download.argtypes = [vp, vp, sz, ctypes.c_int, P(ctypes.c_uint16), P(ctypes.c_uint16), sz]
    lib.zmx_find_longest_match.argtypes = [vp, vp, sz, sz, P(ctypes.c_uint16), P(ctypes.c_uint16),
                                           P(ctypes.c_uint16)]
    lib.zmx_length_array_download.argtypes = [vp, vp, sz, P(ctypes.c_uint16)]
    lib.zmx_hash_links_download.argtypes = [vp, vp, sz, P(ctypes.c_uint16), P(ctypes.c_uint16), P(ctypes.c_uint16)]
    lib.zmx_deflate_range.argtypes = [vp, opt, sz, sz, ctypes.c_int, P(_u8p), P(sz)]
    lib.zmx_checksum.argtypes = [vp, ctypes.c_int, sz, sz, P(ctypes.c_uint32)]
    lib.zmx_checksum_combine.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    lib.zmx_checksum_combine.restype = ctypes.c_uint32
    lib.zmx_chunks_merge.argtypes = [P(vp), P(sz), sz, P(ctypes.c_ubyte), P(_u8p), P(sz)]
    lib.zmx_last_timing.argtypes = [P(ctypes.c_double)]
    lib.zmx_last_kernel_timing.argtypes = [P(ctypes.c_double)]
    lib.zmx_last_host_timing.argtypes = [P(ctypes.c_double)]
    lib.zmx_last_seg_stats.argtypes = [P(ctypes.c_double)]
    lib.zmx_last_match_timing.argtypes = [P(ctypes.c_double)]
    lib.zmx_set_match_kernel.argtypes = [ctypes.c_int]
    if hasattr(lib, "zmx_set_match_order"):   # (absent from an older build selected by ZOPFLI_AMD_LIB for an A/B)
        lib.zmx_set_match_order.argtypes = [ctypes.c_int]
        lib.zmx_set_match_order.restype = ctypes.c_int
    lib.zmx_dist_unique_id.argtypes = [ctypes.c_char_p]
    lib.zmx_dist_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, P(vp)]
    lib.zmx_dist_destroy.argtypes = [vp]
    lib.zmx_dist_destroy.restype = None
    lib.zmx_dist_comm_count.argtypes = [vp]
    lib.zmx_dist_gather.argtypes = [vp, vp, sz, P(vp), P(sz)]
    # (the harness reads the squeeze runs' phase times: last_timing()["dp_kernel"]; a plain caller of the library does not pay for them)
    lib.zmx_set_kernel_timing.argtypes = [ctypes.c_int]
    lib.zmx_set_kernel_timing.restype = None
    lib.zmx_set_kernel_timing(1)
    return lib


def library(path=None):
    """Loads libzopfli_amd.so (built in-tree by __graft_entry__.build()).  No fallback."""
    global _lib
    if path is not None:
        return bind(ctypes.CDLL(path))
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError(f"{LIB} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                               "zopfli_amd has no CPU fallback")
        _lib = bind(ctypes.CDLL(LIB))
    return _lib


def _take(out, size):
    data = ctypes.string_at(out, size.value)
    _libc.free(out)
    return data


def compress(data, fmt=FORMAT_GZIP, options=None, lib=None):
    """ZopfliCompress (zopfli_lib.c:28)."""
    lib = lib or library()
    options = options or ZopfliOptions()
    out, size = _u8p(), ctypes.c_size_t(0)
    lib.ZopfliCompress(ctypes.byref(options), fmt, data, len(data), ctypes.byref(out), ctypes.byref(size))
    return _take(out, size)


def compress_batch(datas, fmt=FORMAT_GZIP, options=None, lib=None):
    """zmx_compress_batch: one ZopfliCompress output per input (a list of bytes), computed in one pass over the
    devices.  Raises RuntimeError with the library's message on failure."""
    lib = lib or library()
    options = options or ZopfliOptions()
    n = len(datas)
    keep = [bytes(d) for d in datas]
    ins = (ctypes.c_char_p * max(n, 1))(*keep)
    sizes = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in keep])
    outs = (_u8p * max(n, 1))()
    outsizes = (ctypes.c_size_t * max(n, 1))()
    # (bound here, not in bind(): a library without the batch entry point — the CPU test library — still loads)
    fn = lib.zmx_compress_batch
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p),
                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_u8p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(options), fmt, n, ins, sizes, outs, outsizes) != 0:
        raise RuntimeError("zmx_compress_batch: " + (lib.zmx_last_error() or b"").decode())
    return [_take(outs[i], ctypes.c_size_t(outsizes[i])) for i in range(n)]


def _device_range(src, nbytes, sync=True):
    """(pointer, bytes) of an integer device pointer with `nbytes`, or of a contiguous tensor-like object (`sync`: a
    torch tensor's current stream is synchronised)."""
    if isinstance(src, int):
        if nbytes is None:
            raise ValueError("a device pointer needs nbytes")
        return src, int(nbytes)
    if not src.is_contiguous():
        raise ValueError("the tensor is not contiguous: its bytes are not one range of device memory")
    size = src.numel() * src.element_size()
    if nbytes is not None and int(nbytes) != size:
        raise ValueError(f"nbytes = {nbytes}, but the tensor holds {size} bytes")
    # the data must be complete before the library's own streams read it
    if sync and type(src).__module__.split(".")[0] == "torch":
        import torch
        torch.cuda.current_stream(src.device).synchronize()
    return src.data_ptr(), size


def _pair_range(x):
    """(pointer, bytes) of a contiguous tensor or of an (integer device pointer, nbytes) pair."""
    return _device_range(int(x[0]), x[1]) if isinstance(x, (tuple, list)) else _device_range(x, None)


def _sync_torch(objects):
    """The current stream of every distinct torch device among the torch tensors in `objects`, synchronised once; anything
    else in there — None, an integer pointer, a tuple — is passed over."""
    devices = {}
    for t in objects:
        if type(t).__module__.split(".")[0] == "torch":
            devices[str(t.device)] = t.device
    if devices:
        import torch
        for device in devices.values():
            torch.cuda.current_stream(device).synchronize()


def compress_device(src, nbytes=None, fmt=FORMAT_GZIP, options=None, lib=None):
    """zmx_compress_device: ZopfliCompress of bytes in device memory — `src` is an integer device pointer with `nbytes`,
    or an object with data_ptr(), numel(), element_size() and is_contiguous() (a torch tensor, whose current stream is
    synchronised first).  Raises ValueError for a non-contiguous tensor, RuntimeError with the library's message when the
    library refuses the pointer or fails."""
    lib = lib or library()
    options = options or ZopfliOptions()
    ptr, size = _device_range(src, nbytes)
    out, outsize = _u8p(), ctypes.c_size_t(0)
    # (bound here, not in bind(): a library without the entry point — the CPU test library — still loads)
    fn = lib.zmx_compress_device
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(_u8p),
                   ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(options), fmt, ptr, size, ctypes.byref(out), ctypes.byref(outsize)) != 0:
        raise RuntimeError("zmx_compress_device: " + (lib.zmx_last_error() or b"").decode())
    return _take(out, outsize)


def _device_ranges(srcs):
    """(pointers, sizes) of a list of tensors or (pointer, nbytes) pairs; the current stream of every distinct torch
    device among them is synchronised once."""
    ptrs, sizes, devices = [], [], {}
    for src in srcs:
        if isinstance(src, (tuple, list)):
            ptr, size = _device_range(int(src[0]), src[1])
        else:
            ptr, size = _device_range(src, None, sync=False)
            if type(src).__module__.split(".")[0] == "torch":
                devices[str(src.device)] = src.device
        ptrs.append(ptr)
        sizes.append(size)
    if devices:
        import torch
        for device in devices.values():
            torch.cuda.current_stream(device).synchronize()
    return ptrs, sizes


def compress_device_batch(srcs, fmt=FORMAT_GZIP, options=None, lib=None):
    """zmx_compress_device_batch: one ZopfliCompress output per input in device memory — `srcs` is a list of tensors
    (objects with data_ptr(), numel(), element_size() and is_contiguous(); the current stream of every torch device
    among them is synchronised first) or of (integer device pointer, nbytes) pairs.  Raises ValueError for a
    non-contiguous tensor, RuntimeError with the library's message when the library refuses a pointer or fails."""
    lib = lib or library()
    options = options or ZopfliOptions()
    ptrs, sizes = _device_ranges(srcs)
    n = len(ptrs)
    ins = (ctypes.c_void_p * max(n, 1))(*ptrs)
    insizes = (ctypes.c_size_t * max(n, 1))(*sizes)
    outs = (_u8p * max(n, 1))()
    outsizes = (ctypes.c_size_t * max(n, 1))()
    # (bound here, not in bind(): a library without the entry point — the CPU test library — still loads)
    fn = lib.zmx_compress_device_batch
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_u8p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(options), fmt, n, ins, insizes, outs, outsizes) != 0:
        raise RuntimeError("zmx_compress_device_batch: " + (lib.zmx_last_error() or b"").decode())
    return [_take(outs[i], ctypes.c_size_t(outsizes[i])) for i in range(n)]


class CapacityError(RuntimeError):
    """compress_device_out: the stream does not fit the destination; `needed` is its size in bytes.
    compress_device_batch_out, compress_device_batch_packed: `needed` is the list of all streams' sizes.
    png_encode_device_out, png_optimize_device_out: the file's size; png_encode_device_batch_packed: the list of the files'."""

    def __init__(self, message, needed):
        super().__init__(message)
        self.needed = needed


def compress_device_out(src, dst, fmt=FORMAT_GZIP, options=None, lib=None):
    """zmx_compress_device_to_device: ZopfliCompress of bytes in device memory into device memory.  `src` is a tensor or
    an (integer device pointer, nbytes) pair, as compress_device takes them; `dst` a contiguous tensor or an (integer
    device pointer, capacity) pair on the same device.  Returns the stream's size: its bytes are dst[0, size).  Raises
    ValueError for a non-contiguous tensor, CapacityError (with the size needed, nothing written) when the stream does not
    fit, RuntimeError with the library's message when the library refuses a pointer or fails."""
    lib = lib or library()
    options = options or ZopfliOptions()
    ptr, size = _pair_range(src)
    out, capacity = _pair_range(dst)
    outsize = ctypes.c_size_t(0)
    # (bound here, not in bind(): a library without the entry point — the CPU test library — still loads)
    fn = lib.zmx_compress_device_to_device
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                   ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(options), fmt, ptr, size, out, capacity, ctypes.byref(outsize)) != 0:
        message = "zmx_compress_device_to_device: " + (lib.zmx_last_error() or b"").decode()
        if outsize.value > capacity:
            raise CapacityError(message, int(outsize.value))
        raise RuntimeError(message)
    return int(outsize.value)


def _batch_failure(who, lib, outsizes, n):
    """The error of a failed device-output batch call: CapacityError with the list of sizes needed when the library
    reported them (a destination was too small; nothing was written), else RuntimeError."""
    message = who + ": " + (lib.zmx_last_error() or b"").decode()
    needed = [int(outsizes[i]) for i in range(n)]
    if any(needed):
        return CapacityError(message, needed)
    return RuntimeError(message)


def compress_device_batch_out(srcs, dsts, fmt=FORMAT_GZIP, options=None, lib=None):
    """zmx_compress_device_batch_to_device: one ZopfliCompress stream per input in device memory, each left in device
    memory.  `srcs` as compress_device_batch takes them; `dsts` a list of as many contiguous tensors or (integer device
    pointer, capacity) pairs, all on one device.  Returns the list of the streams' sizes: stream i is dsts[i][0, size).
    Raises ValueError for a non-contiguous tensor or lists of different lengths, CapacityError (`needed`: the list of
    sizes, nothing written anywhere) when a stream does not fit, RuntimeError with the library's message when the library
    refuses a pointer or fails."""
    lib = lib or library()
    options = options or ZopfliOptions()
    if len(srcs) != len(dsts):
        raise ValueError(f"{len(srcs)} inputs, but {len(dsts)} destinations")
    ptrs, sizes = _device_ranges(srcs)
    outs, capacities = _device_ranges(dsts)
    n = len(ptrs)
    outsizes = (ctypes.c_size_t * max(n, 1))()
    # (bound here, not in bind(): a library without the entry point — the CPU test library — still loads)
    fn = lib.zmx_compress_device_batch_to_device
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                   ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(options), fmt, n, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_size_t * max(n, 1))(*sizes),
          (ctypes.c_void_p * max(n, 1))(*outs), (ctypes.c_size_t * max(n, 1))(*capacities), outsizes) != 0:
        raise _batch_failure("zmx_compress_device_batch_to_device", lib, outsizes, n)
    return [int(outsizes[i]) for i in range(n)]


def compress_device_batch_packed(srcs, arena, align=1, fmt=FORMAT_GZIP, options=None, lib=None):
    """zmx_compress_device_batch_packed: the same streams packed into `arena`, a contiguous tensor or an (integer device
    pointer, capacity) pair: stream i begins at the end of stream i - 1 rounded up to `align` (a power of two, 1 .. 4096);
    the bytes between streams are not written.  Returns (offsets, sizes).  Raises as compress_device_batch_out does; a
    CapacityError's `needed` is the list of sizes, from which compress_batch_bound or the offsets' rule gives the arena."""
    lib = lib or library()
    options = options or ZopfliOptions()
    ptrs, sizes = _device_ranges(srcs)
    out, capacity = _pair_range(arena)
    n = len(ptrs)
    offsets = (ctypes.c_size_t * max(n, 1))()
    outsizes = (ctypes.c_size_t * max(n, 1))()
    fn = lib.zmx_compress_device_batch_packed
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                   ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(options), fmt, n, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_size_t * max(n, 1))(*sizes),
          out, capacity, int(align), offsets, outsizes) != 0:
        raise _batch_failure("zmx_compress_device_batch_packed", lib, outsizes, n)
    return [int(offsets[i]) for i in range(n)], [int(outsizes[i]) for i in range(n)]


def compress_batch_bound(sizes, fmt=FORMAT_GZIP, align=1, lib=None):
    """zmx_compress_batch_bound: an arena capacity that does for compress_device_batch_packed of inputs of these sizes."""
    lib = lib or library()
    fn = lib.zmx_compress_batch_bound
    fn.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t]
    fn.restype = ctypes.c_size_t
    n = len(sizes)
    return int(fn(fmt, n, (ctypes.c_size_t * max(n, 1))(*[int(s) for s in sizes]), int(align)))


def compress_bound(nbytes, fmt=FORMAT_GZIP, lib=None):
    """zmx_compress_bound: a destination capacity that does for any input of `nbytes` bytes."""
    lib = lib or library()
    fn = lib.zmx_compress_bound
    fn.argtypes = [ctypes.c_int, ctypes.c_size_t]
    fn.restype = ctypes.c_size_t
    return int(fn(fmt, nbytes))


INFLATE_STATUS = ["OK", "HEADER", "DICT", "BLOCK_TYPE", "STORED_LEN", "TOO_MANY_SYMBOLS", "REPEAT", "OVERSUBSCRIBED", "INCOMPLETE",
                  "NO_END_CODE", "BAD_CODE", "BAD_SYMBOL", "DISTANCE", "TRUNCATED", "CAPACITY", "CHECKSUM", "SIZE"]   # ZMX_INFLATE_*
INFLATE_OK, INFLATE_CAPACITY = 0, 14
ERR_DATA = 4   # ZMX_ERR_DATA


class InflateResult(ctypes.Structure):
    """zmx_inflate_result."""
    _fields_ = [("outsize", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("status", ctypes.c_uint32), ("block", ctypes.c_uint32),
                ("stored_check", ctypes.c_uint32), ("stored_isize", ctypes.c_uint32)]

    def astuple(self):
        return (int(self.outsize), int(self.consumed), int(self.status), int(self.block), int(self.stored_check), int(self.stored_isize))


class InflateError(RuntimeError):
    """inflate_device_batch, inflate_device, inflate_size_device: stream `index` is no valid stream — `status` (a
    ZMX_INFLATE_* number; INFLATE_STATUS names it) in deflate block `block`; `needed`: the bytes it decoded to up to
    there.  `results`: the InflateResult of every stream of the call."""

    def __init__(self, index, status, block, needed, message="", results=None):
        super().__init__(message or f"stream {index}: ZMX_INFLATE_{INFLATE_STATUS[status] if status < len(INFLATE_STATUS) else status}")
        self.index, self.status, self.block, self.needed = index, status, block, needed
        self.results = results or []


def _inflate_format(fmt):
    if isinstance(fmt, str):
        return {"gzip": FORMAT_GZIP, "zlib": FORMAT_ZLIB, "deflate": FORMAT_DEFLATE}[fmt]
    return int(fmt)


def _inflate_call(lib, fn, who, ctx_args, fmt, streams, outs):
    """One inflate entry: `outs` None for the size-only mode, else a list of tensors, (pointer, capacity) pairs or None.
    Returns (rc, results, capacities)."""
    ptrs, sizes = _device_ranges(streams)
    n = len(ptrs)
    if outs is not None and len(outs) != n:
        raise ValueError(f"{n} streams, but {len(outs)} destinations")
    out_ptrs, capacities = [None] * n, [0] * n
    if outs is not None:
        given = [i for i in range(n) if outs[i] is not None]
        got_ptrs, got_caps = _device_ranges([outs[i] for i in given])
        for i, p, c in zip(given, got_ptrs, got_caps):
            # (a destination of no bytes still asks for the stored mode: any non-null pointer goes with a size of 0)
            out_ptrs[i], capacities[i] = p or 1, c
    results = (InflateResult * max(n, 1))()
    P, sz, vp = ctypes.POINTER, ctypes.c_size_t, ctypes.c_void_p
    fn.argtypes = [vp] * len(ctx_args) + [ctypes.c_int, sz, P(vp), P(sz), P(vp), P(sz), P(InflateResult)]
    fn.restype = ctypes.c_int
    rc = fn(*ctx_args, _inflate_format(fmt), n, (vp * max(n, 1))(*ptrs), (sz * max(n, 1))(*sizes),
            (vp * max(n, 1))(*out_ptrs) if outs is not None else None, (sz * max(n, 1))(*capacities), results)
    found = [results[i] for i in range(n)]
    if rc != 0 and all(r.status == INFLATE_OK for r in found):
        raise RuntimeError(who + ": " + (lib.zmx_last_error() or b"").decode())
    return rc, found, capacities


def _inflate_raise(lib, who, results, single):
    """The error of a failed pooled inflate call: CapacityError (`needed`: the size, or the list of all streams' sizes)
    where the first failing stream only lacks room, else InflateError."""
    message = who + ": " + (lib.zmx_last_error() or b"").decode()
    index = next(i for i, r in enumerate(results) if r.status != INFLATE_OK)
    r = results[index]
    if r.status == INFLATE_CAPACITY:
        raise CapacityError(message, int(r.outsize) if single else [int(x.outsize) for x in results])
    raise InflateError(index, int(r.status), int(r.block), int(r.outsize), message, results)


def inflate_size_device(streams, format="gzip", lib=None):
    """zmx_inflate_device_batch in its size-only mode: the bytes every stream decodes to, nothing stored (and so no checksum
    compared).  `streams`: uint8 tensors or (integer device pointer, nbytes) pairs.  Raises InflateError."""
    lib = lib or library()
    rc, results, _ = _inflate_call(lib, lib.zmx_inflate_device_batch, "zmx_inflate_device_batch", [], format, streams, None)
    if rc != 0:
        _inflate_raise(lib, "zmx_inflate_device_batch", results, False)
    return [int(r.outsize) for r in results]


def inflate_device_batch(streams, format="gzip", outs=None, lib=None):
    """zmx_inflate_device_batch: every deflate / zlib / gzip stream of `streams` (uint8 tensors or (integer device pointer,
    nbytes) pairs, all on one device) decoded into device memory in one launch, checksums verified on the device.  With
    `outs` (as many contiguous tensors or (pointer, capacity) pairs) stream i goes to outs[i]; without, a size-only call
    comes first and the outputs are allocated.  Returns the outputs as uint8 tensors of exactly the decoded sizes (views of
    `outs` where they are tensors; (pointer, size) pairs where they are pairs).  Raises InflateError for the first stream
    that is no valid stream (all results in `.results`), CapacityError (`needed`: the list of sizes) where one does not fit,
    RuntimeError with the library's message for a refused pointer or a device failure."""
    lib = lib or library()
    n = len(streams)
    if outs is None:
        import torch
        sizes = inflate_size_device(streams, format, lib)
        devices = [s.device for s in streams if not isinstance(s, (tuple, list))]
        outs = [torch.empty(size, dtype=torch.uint8, device=devices[0] if devices else "cuda") for size in sizes]
    rc, results, _ = _inflate_call(lib, lib.zmx_inflate_device_batch, "zmx_inflate_device_batch", [], format, streams, outs)
    if rc != 0:
        _inflate_raise(lib, "zmx_inflate_device_batch", results, False)
    made = []
    for i in range(n):
        size = int(results[i].outsize)
        made.append((int(outs[i][0]), size) if isinstance(outs[i], (tuple, list)) else outs[i].view(-1)[:size])
    return made


def inflate_device(stream, format="gzip", out=None, size=None, lib=None):
    """zmx_inflate_device_batch of one stream: a uint8 tensor or an (integer device pointer, nbytes) pair.  `out`: a tensor
    or (pointer, capacity) pair to decode into; without one the output is allocated — `size` bytes where the caller knows
    the size, else after a size-only call.  Returns a uint8 tensor of exactly the decoded size.  Raises as
    inflate_device_batch does; CapacityError's `needed` is the size."""
    lib = lib or library()
    if out is None and size is not None:
        import torch
        out = torch.empty(int(size), dtype=torch.uint8, device="cuda" if isinstance(stream, (tuple, list)) else stream.device)
    try:
        return inflate_device_batch([stream], format, None if out is None else [out], lib)[0]
    except CapacityError as e:
        raise CapacityError(str(e), e.needed[0]) from None


PNG_DECODE_STATUS = ["OK", "SIGNATURE", "IHDR", "INTERLACE", "CHUNK", "CRITICAL", "CRC", "PLTE", "TRNS", "STREAM", "SIZE", "FILTER",
                     "CAPACITY", "SHAPE"]   # ZMX_PNG_DECODE_*
PNG_DECODE_OK, PNG_DECODE_CAPACITY, PNG_DECODE_SHAPE = 0, 12, 13
PNG_DECODE_OWN, PNG_DECODE_RGBA8 = 0, 1


class PngDecodeResult(ctypes.Structure):
    """zmx_png_decode_result: what a decode or info call says of one file."""
    _fields_ = [("status", ctypes.c_uint32), ("detail", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("colortype", ctypes.c_uint32), ("bitdepth", ctypes.c_uint32), ("interlace", ctypes.c_uint32), ("palettesize", ctypes.c_uint32),
                ("has_key", ctypes.c_uint32), ("key_r", ctypes.c_uint32), ("key_g", ctypes.c_uint32), ("key_b", ctypes.c_uint32),
                ("outsize", ctypes.c_uint64), ("outsize_own", ctypes.c_uint64), ("outsize_rgba8", ctypes.c_uint64),
                ("palette_bytes", ctypes.c_ubyte * 1024)]

    @property
    def palette(self):
        """the palette's r, g, b, a bytes, four an entry (empty without a PLTE)"""
        return bytes(self.palette_bytes[:4 * int(self.palettesize)])

    @property
    def key(self):
        """the tRNS key of colour types 0 and 2 as (r, g, b) at the file's depth, or None"""
        return (int(self.key_r), int(self.key_g), int(self.key_b)) if self.has_key else None

    @property
    def linebytes(self):
        return int(self.outsize_own) // max(int(self.height), 1)

    def astuple(self):
        return tuple(int(getattr(self, name)) for name, _ in self._fields_[:15]) + (bytes(self.palette_bytes),)

    def own_shape(self):
        """the shape of the OWN mode's uint8 tensor: (H, linebytes) for palette images and grey below 8 bits, else
        (H, W, channels * bitdepth / 8)"""
        if self.colortype == 3 or self.bitdepth < 8:
            return (int(self.height), self.linebytes)
        return (int(self.height), int(self.width), self.linebytes // int(self.width))


class PngDecodeError(RuntimeError):
    """png_decode_device*, png_info_device: file `index` is no PNG the library decodes — `status` (a ZMX_PNG_DECODE_* number;
    PNG_DECODE_STATUS names it) with its `detail`.  `results`: the PngDecodeResult of every file of the call."""

    def __init__(self, index, status, detail, message="", results=None):
        super().__init__(message or f"file {index}: ZMX_PNG_DECODE_{PNG_DECODE_STATUS[status] if status < len(PNG_DECODE_STATUS) else status}")
        self.index, self.status, self.detail = index, status, detail
        self.results = results or []


def _png_decode_mode(mode):
    if isinstance(mode, str):
        return {"own": PNG_DECODE_OWN, "rgba8": PNG_DECODE_RGBA8}[mode]
    return int(mode)


def _png_decode_call(lib, fn, who, ctx_args, mode, files, outs, tail=()):
    """One decode entry: `mode` None for the info entry (no mode, no destinations); `outs` None for the size-only mode, else
    a list of tensors, (pointer, capacity) pairs or None.  Returns (rc, results)."""
    ptrs, sizes = _device_ranges(files)
    n = len(ptrs)
    if outs is not None and len(outs) != n:
        raise ValueError(f"{n} files, but {len(outs)} destinations")
    results = (PngDecodeResult * max(n, 1))()
    P, sz, vp = ctypes.POINTER, ctypes.c_size_t, ctypes.c_void_p
    args = list(ctx_args)
    types = [vp] * len(ctx_args)
    if mode is not None:
        args.append(_png_decode_mode(mode))
        types.append(ctypes.c_int)
    args += [n, (vp * max(n, 1))(*ptrs), (sz * max(n, 1))(*sizes)]
    types += [sz, P(vp), P(sz)]
    if mode is not None:
        out_ptrs, capacities = [None] * n, [0] * n
        if outs is not None:
            given = [i for i in range(n) if outs[i] is not None]
            got_ptrs, got_caps = _device_ranges([outs[i] for i in given])
            for i, p, c in zip(given, got_ptrs, got_caps):
                out_ptrs[i], capacities[i] = p or 1, c
        args += [(vp * max(n, 1))(*out_ptrs) if outs is not None else None, (sz * max(n, 1))(*capacities)]
        types += [P(vp), P(sz)]
    fn.argtypes = types + [P(PngDecodeResult)] + [t for t, _ in tail]
    fn.restype = ctypes.c_int
    rc = fn(*args, results, *[v for _, v in tail])
    found = [results[i] for i in range(n)]
    if rc != 0 and all(r.status == PNG_DECODE_OK for r in found):
        raise RuntimeError(who + ": " + (lib.zmx_last_error() or b"").decode())
    return rc, found


def _png_decode_raise(lib, who, results, single):
    """The error of a failed decode call: CapacityError where the first failing file only lacks room, else PngDecodeError."""
    message = who + ": " + (lib.zmx_last_error() or b"").decode()
    index = next(i for i, r in enumerate(results) if r.status != PNG_DECODE_OK)
    r = results[index]
    if r.status == PNG_DECODE_CAPACITY:
        raise CapacityError(message, int(r.outsize) if single else [int(x.outsize) for x in results])
    raise PngDecodeError(index, int(r.status), int(r.detail), message, results)


def png_info_device(files, lib=None, check=True):
    """zmx_png_info_device: the chunk walk of every PNG file of `files` (uint8 tensors or (integer device pointer, nbytes)
    pairs, all on one device), the chunks' CRCs compared, nothing decoded.  Returns the list of PngDecodeResult — width,
    height, colortype, bitdepth, interlace, palette, key, status, the sizes of both modes.  Raises PngDecodeError for the
    first file that is none (`check` False: returns the results whatever their statuses)."""
    lib = lib or library()
    rc, results = _png_decode_call(lib, lib.zmx_png_info_device, "zmx_png_info_device", [], None, files, None)
    if rc != 0 and check:
        _png_decode_raise(lib, "zmx_png_info_device", results, False)
    return results


def _png_decode_views(mode, results, outs):
    made = []
    rgba = _png_decode_mode(mode) == PNG_DECODE_RGBA8
    for r, out in zip(results, outs):
        if isinstance(out, (tuple, list)):
            made.append((int(out[0]), int(r.outsize)))
            continue
        shape = (int(r.height), int(r.width), 4) if rgba else r.own_shape()
        made.append(out.view(-1)[:int(r.outsize)].view(shape))
    return made


def png_decode_device_batch(files, mode="rgba8", outs=None, lib=None):
    """zmx_png_decode_device_batch: every PNG file of `files` (uint8 tensors or (integer device pointer, nbytes) pairs, all on
    one device) decoded into device memory: the chunk walk, the inflate and the unfilter on the device, no byte on the host.
    `mode`: "own" — the file's colour type and depth in the layout the encode entries read — or "rgba8".  With `outs` (as
    many contiguous tensors or (pointer, capacity) pairs) file i goes to outs[i]; without, one png_info_device round sizes
    the tensors.  Returns (infos, tensors): uint8 tensors shaped (H, W, 4) for "rgba8"; for "own" (H, linebytes) for palette
    and low-bit images and (H, W, channels * depth / 8) otherwise ((pointer, size) pairs where `outs` holds pairs).  Raises
    PngDecodeError for the first bad file (all results in `.results`), CapacityError (`needed`: the list of sizes) where
    one does not fit, RuntimeError for a refused pointer or a device failure.
    `outs` may also hold PngSinks, one per file (zmx_png_decode_sink_device_batch): file i is decoded into the tensor of
    outs[i] as it lies — strided, planar, float, 16-bit —, `mode` is ignored, and (infos, the sinks' tensors) comes back.
    A file whose size is not its sink's ends PNG_DECODE_SHAPE.  A list that mixes sinks and tensors is a ValueError."""
    lib = lib or library()
    if outs is not None and _png_are_sinks(outs):
        rc, results = _png_decode_sink_call(lib, lib.zmx_png_decode_sink_device_batch, "zmx_png_decode_sink_device_batch", [], files, outs)
        if rc != 0:
            _png_decode_raise(lib, "zmx_png_decode_sink_device_batch", results, False)
        return results, [s.tensor for s in outs]
    if outs is None:
        import torch
        infos = png_info_device(files, lib)
        key = "outsize_rgba8" if _png_decode_mode(mode) == PNG_DECODE_RGBA8 else "outsize_own"
        devices = [f.device for f in files if not isinstance(f, (tuple, list))]
        outs = [torch.empty(int(getattr(r, key)), dtype=torch.uint8, device=devices[0] if devices else "cuda") for r in infos]
    rc, results = _png_decode_call(lib, lib.zmx_png_decode_device_batch, "zmx_png_decode_device_batch", [], mode, files, outs)
    if rc != 0:
        _png_decode_raise(lib, "zmx_png_decode_device_batch", results, False)
    return results, _png_decode_views(mode, results, outs)


def png_decode_device(file, mode="rgba8", out=None, lib=None):
    """png_decode_device_batch of one file.  Returns (info, tensor); CapacityError's `needed` is the size.  `out` may be a
    PngSink (zmx_png_decode_sink_device)."""
    if isinstance(out, PngSink):
        lib = lib or library()
        (ptr,), (size,) = _device_ranges([file])
        _sync_torch([out.tensor])
        result = PngDecodeResult()
        fn = lib.zmx_png_decode_sink_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(PngSinkStruct), ctypes.POINTER(PngDecodeResult)]
        fn.restype = ctypes.c_int
        if fn(ptr, size, ctypes.byref(out.struct), ctypes.byref(result)) != 0:
            if result.status == PNG_DECODE_OK:
                raise RuntimeError("zmx_png_decode_sink_device: " + (lib.zmx_last_error() or b"").decode())
            _png_decode_raise(lib, "zmx_png_decode_sink_device", [result], True)
        return result, out.tensor
    try:
        infos, made = png_decode_device_batch([file], mode, None if out is None else [out], lib)
    except CapacityError as e:
        raise CapacityError(str(e), e.needed[0]) from None
    return infos[0], made[0]


def png_decode_size_device(files, mode="rgba8", lib=None):
    """zmx_png_decode_device_batch in its size-only mode: the walk, the CRCs and the stream's size check, nothing stored (the
    Adler-32 is not compared).  Returns the list of PngDecodeResult; raises PngDecodeError."""
    lib = lib or library()
    rc, results = _png_decode_call(lib, lib.zmx_png_decode_device_batch, "zmx_png_decode_device_batch", [], mode, files, None)
    if rc != 0:
        _png_decode_raise(lib, "zmx_png_decode_device_batch", results, False)
    return results


class PngDecodeHooks(ctypes.Structure):
    """zmx_png_decode_hooks."""
    _fields_ = [("force_wide", ctypes.c_int), ("idat_capacity", ctypes.c_uint32)]


class PngImage(ctypes.Structure):
    """zmx_png_image"""
    _fields_ = [("d_pixels", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("colortype", ctypes.c_uint32), ("bitdepth", ctypes.c_uint32)]


# ZMX_PNG_FILTER_*: zopflipng's --filters= letters, "p" for predefined types, "auto" for zopflipng's own choice
PNG_STRATEGIES = {"0": 0, "1": 1, "2": 2, "3": 3, "4": 4, "m": 5, "e": 6, "b": 7, "p": 8, "auto": 10}
PNG_FILTER_MINSUM, PNG_FILTER_ENTROPY, PNG_FILTER_BRUTE, PNG_FILTER_PREDEFINED = 5, 6, 7, 8
PNG_FILTER_AUTO = 10   # zopflipng without --filters: the strategy of its trials (Context.png_choose_strategy_device)
_PNG_COLORTYPE = {1: 0, 2: 4, 3: 2, 4: 6}   # channels -> grey, grey + alpha, RGB, RGBA


def _png_strategy(strategy):
    return PNG_STRATEGIES[strategy] if isinstance(strategy, str) else int(strategy)


PNG_LOSSY_TRANSPARENT, PNG_LOSSY_8BIT = 1, 2   # ZMX_PNG_LOSSY_*


def _png_lossy(lossy_transparent, lossy_8bit):
    return (PNG_LOSSY_TRANSPARENT if lossy_transparent else 0) | (PNG_LOSSY_8BIT if lossy_8bit else 0)


_size_p = ctypes.POINTER(ctypes.c_size_t)
_PNG_TO_HOST = [ctypes.POINTER(_u8p), _size_p]                                     # out, outsize
_PNG_TO_DEVICE = [ctypes.c_void_p, ctypes.c_size_t, _size_p]                       # d_out, capacity, outsize
_PNG_PACKED = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, _size_p, _size_p]   # d_arena, capacity, align, outoffset, outsize


def _png_entry(lib, name, struct, lossy, batch, tail, suffixed=False):
    """(function, the arguments between the strategy or the types and `tail`) of a PNG entry on images of type `struct`:
    its flags.  `suffixed`: the entry has a plain symbol without flags and a _lossy one with them; the _lossy symbol is
    bound only where flags are set — a library from before the flags still loads and serves lossy = 0.
    (bound here, at call time, not in bind(): a library without the entry point — the CPU test library — still loads)"""
    takes_flags = bool(lossy) or not suffixed
    fn = getattr(lib, name + "_lossy" if suffixed and lossy else name)
    head = ([ctypes.POINTER(ZopfliOptions), ctypes.c_size_t, ctypes.POINTER(struct), ctypes.c_int] if batch else
            [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(struct), ctypes.c_int, ctypes.c_char_p])
    fn.argtypes = head + ([ctypes.c_uint] if takes_flags else []) + tail
    fn.restype = ctypes.c_int
    return fn, ((lossy,) if takes_flags else ())


# The four shapes of a PNG entry.  `name`: the symbol (without _lossy); `struct`: PngImage, PngIndexImage or
# PngSourceStruct; `im` / `ims`: one such struct, or a list of them.
def _png_single(name, struct, im, strategy, options, types, lib, lossy, suffixed=False):
    """one image -> the file's bytes"""
    lib = lib or library()
    options = options or ZopfliOptions()
    out, outsize = _u8p(), ctypes.c_size_t(0)
    fn, flags = _png_entry(lib, name, struct, lossy, False, _PNG_TO_HOST, suffixed)
    if fn(ctypes.byref(options), ctypes.byref(im), _png_strategy(strategy), types, *flags, ctypes.byref(out), ctypes.byref(outsize)) != 0:
        raise RuntimeError(name + ": " + (lib.zmx_last_error() or b"").decode())
    return _take(out, outsize)


def _png_single_out(name, struct, im, dst, strategy, options, types, lib, lossy):
    """one image -> the file in `dst`; its size"""
    lib = lib or library()
    options = options or ZopfliOptions()
    out, capacity = _pair_range(dst)
    outsize = ctypes.c_size_t(0)
    fn, flags = _png_entry(lib, name, struct, lossy, False, _PNG_TO_DEVICE)
    if fn(ctypes.byref(options), ctypes.byref(im), _png_strategy(strategy), types, *flags, out, capacity, ctypes.byref(outsize)) != 0:
        message = name + ": " + (lib.zmx_last_error() or b"").decode()
        if outsize.value > capacity:
            raise CapacityError(message, int(outsize.value))
        raise RuntimeError(message)
    return int(outsize.value)


def _png_batch(name, struct, ims, strategy, options, lib, lossy, suffixed=False):
    """a list of images -> the list of the files' bytes"""
    lib = lib or library()
    options = options or ZopfliOptions()
    n = len(ims)
    outs = (_u8p * max(n, 1))()
    outsizes = (ctypes.c_size_t * max(n, 1))()
    fn, flags = _png_entry(lib, name, struct, lossy, True, _PNG_TO_HOST, suffixed)
    if fn(ctypes.byref(options), n, (struct * max(n, 1))(*ims), _png_strategy(strategy), *flags, outs, outsizes) != 0:
        raise RuntimeError(name + ": " + (lib.zmx_last_error() or b"").decode())
    return [_take(outs[i], ctypes.c_size_t(outsizes[i])) for i in range(n)]


def _png_batch_packed(name, struct, ims, arena, align, strategy, options, lib, lossy):
    """a list of images -> the files packed into `arena`; (offsets, sizes)"""
    lib = lib or library()
    options = options or ZopfliOptions()
    out, capacity = _pair_range(arena)
    n = len(ims)
    offsets = (ctypes.c_size_t * max(n, 1))()
    outsizes = (ctypes.c_size_t * max(n, 1))()
    fn, flags = _png_entry(lib, name, struct, lossy, True, _PNG_PACKED)
    if fn(ctypes.byref(options), n, (struct * max(n, 1))(*ims), _png_strategy(strategy), *flags, out, capacity, int(align), offsets, outsizes) != 0:
        raise _batch_failure(name, lib, outsizes, n)
    return [int(offsets[i]) for i in range(n)], [int(outsizes[i]) for i in range(n)]


def _png_types(predefined, height):
    types = None if predefined is None else bytes(bytearray(int(t) for t in predefined))
    if types is not None and len(types) != height:
        raise ValueError(f"{len(types)} predefined types for {height} rows")
    return types


class PngLossyInfo(ctypes.Structure):
    """zmx_png_lossy_info; first_transparent is 2^64 - 1 without a transparent pixel."""
    _fields_ = [("mode", ctypes.c_uint32), ("partial_alpha", ctypes.c_uint32), ("numcolors", ctypes.c_uint32), ("fill_r", ctypes.c_uint32),
                ("fill_g", ctypes.c_uint32), ("fill_b", ctypes.c_uint32), ("first_transparent", ctypes.c_uint64)]


def _png_image(image, sync=True):
    """The zmx_png_image of a contiguous uint8 tensor (H, W) or (H, W, 2 | 3 | 4), or of a tuple
    (pointer, width, height, colortype, bitdepth)."""
    if isinstance(image, (tuple, list)):
        ptr, width, height, colortype, bitdepth = image
        return PngImage(int(ptr) or None, int(width), int(height), int(colortype), int(bitdepth))
    shape = tuple(image.shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3 or shape[2] not in _PNG_COLORTYPE or image.element_size() != 1:
        raise ValueError("an image tensor is uint8 of shape (H, W) or (H, W, 2 | 3 | 4); 16-bit data goes as "
                         "(pointer, width, height, colortype, bitdepth)")
    ptr, _ = _device_range(image, None, sync=sync)
    return PngImage(ptr or None, shape[1], shape[0], _PNG_COLORTYPE[shape[2]], 8)


PNG_SAMPLE_U8, PNG_SAMPLE_U16, PNG_SAMPLE_F16, PNG_SAMPLE_BF16, PNG_SAMPLE_F32 = 0, 1, 2, 3, 4   # ZMX_PNG_SAMPLE_*
_PNG_SAMPLE_OF_DTYPE = {"uint8": PNG_SAMPLE_U8, "uint16": PNG_SAMPLE_U16, "float16": PNG_SAMPLE_F16, "bfloat16": PNG_SAMPLE_BF16,
                        "float32": PNG_SAMPLE_F32}


class PngSourceStruct(ctypes.Structure):
    """zmx_png_source"""
    _fields_ = [("d_data", ctypes.c_void_p), ("stride_y", ctypes.c_int64), ("stride_x", ctypes.c_int64), ("stride_c", ctypes.c_int64),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("channels", ctypes.c_uint32), ("sample", ctypes.c_uint32),
                ("bitdepth", ctypes.c_uint32), ("order", ctypes.c_uint8 * 4)]


class PngSource:
    """A zmx_png_source: an image as a GPU program holds it, for the png_* functions in an image's place.
    `data`: a torch tensor of dtype uint8, uint16, float16, bfloat16 or float32 on the device, contiguous or not — a crop, a
    [::2] view, a flip, an expand() all do; its strides are taken as they are, in bytes — of shape (H, W, C) or (H, W) with
    layout "HWC", (C, H, W) or (H, W) with "CHW", C from 1 to 4; or a tuple that spells out the struct: (pointer, stride_y,
    stride_x, stride_c, width, height, channels, sample, bitdepth[, order]).  Floats are taken as [0, 1] and quantised as
    torchvision does: mul(maxv).add_(0.5).clamp_(0, maxv).to(int).  `order`: "RGBA" (the channels as they lie), "BGRA" (the
    first three reversed) or a permutation: PNG channel k is the tensor's channel order[k].  `bitdepth`: of the PNG, 8 or 16;
    None: 16 for uint16, else 8 (uint8 -> 16 and uint16 -> 8 are refused by the library).  Nothing is copied; the object
    keeps the tensor alive."""

    def __init__(self, data, layout="HWC", order="RGBA", bitdepth=None):
        self.tensor = None
        if isinstance(data, (tuple, list)):
            ptr, sy, sx, sc, width, height, channels, sample, depth = data[:9]
            if len(data) > 9:
                order = data[9]
            depth = int(depth)
        else:
            dtype = str(data.dtype).split(".")[-1]
            if dtype not in _PNG_SAMPLE_OF_DTYPE:
                raise ValueError(f"a source tensor is uint8, uint16, float16, bfloat16 or float32, not {dtype}")
            if layout not in ("HWC", "CHW"):
                raise ValueError(f'layout is "HWC" or "CHW", not {layout!r}')
            shape, esize = tuple(data.shape), data.element_size()
            strides = tuple(int(s) * esize for s in data.stride())
            if len(shape) == 2:
                shape, strides = (shape + (1,), strides + (esize,)) if layout == "HWC" else ((1,) + shape, (esize,) + strides)
            if len(shape) != 3:
                raise ValueError("a source tensor has two or three dimensions (png_sources takes a batch)")
            (height, width, channels), (sy, sx, sc) = (shape, strides) if layout == "HWC" else (
                (shape[1], shape[2], shape[0]), (strides[1], strides[2], strides[0]))
            if not 1 <= channels <= 4:
                raise ValueError(f"{channels} channels: an image has 1 to 4")
            sample = _PNG_SAMPLE_OF_DTYPE[dtype]
            depth = (16 if sample == PNG_SAMPLE_U16 else 8) if bitdepth is None else int(bitdepth)
            ptr = data.data_ptr()
            self.tensor = data
        channels = int(channels)
        if isinstance(order, str):
            if order not in ("RGBA", "BGRA"):
                raise ValueError(f'order is "RGBA", "BGRA" or a permutation, not {order!r}')
            order = tuple(range(channels)) if order == "RGBA" or channels < 3 else (2, 1, 0, 3)[:channels]
        order = tuple(int(k) for k in order)
        if len(order) < channels or len(order) > 4:
            raise ValueError(f"order names {len(order)} channels, the image has {channels}")
        self.struct = PngSourceStruct(int(ptr) or None, int(sy), int(sx), int(sc), int(width), int(height), channels, int(sample), depth,
                                      (ctypes.c_uint8 * 4)(*(order + (0,) * (4 - len(order)))))

    @property
    def height(self):
        return int(self.struct.height)


def png_sources(batch, layout="NCHW", order="RGBA", bitdepth=None):
    """The PngSources of a batch tensor (N, C, H, W) or (N, H, W, C) — layout "NCHW" or "NHWC" —, one per image, views
    without a copy: for the _batch functions."""
    if layout not in ("NCHW", "NHWC"):
        raise ValueError(f'layout is "NCHW" or "NHWC", not {layout!r}')
    return [PngSource(batch[i], layout[1:], order, bitdepth) for i in range(batch.shape[0])]


class PngSinkStruct(ctypes.Structure):
    """zmx_png_sink"""
    _fields_ = PngSourceStruct._fields_


class PngSink(PngSource):
    """A zmx_png_sink: where a decoded image goes, as a GPU program holds it — for `outs` of png_decode_device_batch and
    Context.png_decode_device, and for Context.png_unpack_device.  `data`: a writable torch tensor of dtype uint8, uint16,
    float16, bfloat16 or float32 on the device, contiguous or not, its strides taken as they are, shaped as PngSource's;
    or the tuple that spells out the struct.  The channels say what is asked for: 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA;
    PNG channel k goes to the tensor's channel order[k] ("BGRA": the first three reversed).  `bitdepth`: of the values, 8
    or 16; None: 16 for uint16, else 8.  Integers hold the value, floats value / 255 or value / 65535 (one fp32 division,
    rounded to nearest-even into float16 and bfloat16).  No two samples may share a byte: an expand() is refused.  The
    object keeps the tensor alive."""

    def __init__(self, data, layout="HWC", order="RGBA", bitdepth=None):
        super().__init__(data, layout, order, bitdepth)
        self.struct = PngSinkStruct.from_buffer_copy(self.struct)


def png_sinks(batch, layout="NCHW", order="RGBA", bitdepth=None):
    """The PngSinks of a batch tensor (N, C, H, W) or (N, H, W, C) — layout "NCHW" or "NHWC" —, one per image, views without
    a copy: a batch of files decoded into one tensor."""
    if layout not in ("NCHW", "NHWC"):
        raise ValueError(f'layout is "NCHW" or "NHWC", not {layout!r}')
    return [PngSink(batch[i], layout[1:], order, bitdepth) for i in range(batch.shape[0])]


def _png_are_sinks(outs):
    """Whether a list of destinations holds PngSinks (all of it: a mixed list is an error)."""
    kinds = {isinstance(out, PngSink) for out in outs}
    if kinds == {True, False}:
        raise ValueError("a list of destinations holds PngSinks or tensors, not both")
    return kinds == {True}


def _png_sink_array(sinks):
    n = len(sinks)
    return (PngSinkStruct * max(n, 1))(*[s.struct for s in sinks])


def png_sink_check(sink, lib=None):
    """zmx_png_sink_check: RuntimeError with the library's message for a PngSink the entries refuse without asking the
    runtime about its memory — host arithmetic."""
    lib = lib or library()
    fn = lib.zmx_png_sink_check
    fn.argtypes = [ctypes.POINTER(PngSinkStruct)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(sink.struct)) != 0:
        raise RuntimeError((lib.zmx_last_error() or b"").decode())


def _png_decode_sink_call(lib, fn, who, ctx_args, files, sinks, tail=()):
    """One decode entry that takes sinks.  Returns (rc, results)."""
    ptrs, sizes = _device_ranges(files)
    n = len(ptrs)
    if len(sinks) != n:
        raise ValueError(f"{n} files, but {len(sinks)} sinks")
    _sync_torch(s.tensor for s in sinks)
    results = (PngDecodeResult * max(n, 1))()
    P, sz, vp = ctypes.POINTER, ctypes.c_size_t, ctypes.c_void_p
    fn.argtypes = [vp] * len(ctx_args) + [sz, P(vp), P(sz), P(PngSinkStruct), P(PngDecodeResult)] + [t for t, _ in tail]
    fn.restype = ctypes.c_int
    rc = fn(*ctx_args, n, (vp * max(n, 1))(*ptrs), (sz * max(n, 1))(*sizes), _png_sink_array(sinks), results, *[v for _, v in tail])
    found = [results[i] for i in range(n)]
    if rc != 0 and all(r.status == PNG_DECODE_OK for r in found):
        raise RuntimeError(who + ": " + (lib.zmx_last_error() or b"").decode())
    return rc, found


def png_decode_tensors(files, dtype=None, channels=3, layout="NCHW", bitdepth=None, lib=None):
    """The loader's call: PNG files of ONE size in device memory (what png_decode_device_batch takes) decoded into one batch
    tensor (N, channels, H, W) — layout "NHWC": (N, H, W, channels) — of `dtype` (default torch.float32): one
    png_info_device round, one tensor, one decode call with a PngSink per image.  channels 1 .. 4: grey, grey + alpha, RGB,
    RGBA, whatever the files' own colour types; `bitdepth` as PngSink's.  Returns (infos, tensor).  ValueError names the
    first file whose size is not the first file's; PngDecodeError as png_decode_device_batch."""
    import torch
    lib = lib or library()
    if layout not in ("NCHW", "NHWC"):
        raise ValueError(f'layout is "NCHW" or "NHWC", not {layout!r}')
    dtype = dtype or torch.float32
    infos = png_info_device(files, lib)
    devices = [f.device for f in files if not isinstance(f, (tuple, list))]
    device = devices[0] if devices else "cuda"
    if not infos:
        return [], torch.empty((0, channels, 0, 0) if layout == "NCHW" else (0, 0, 0, channels), dtype=dtype, device=device)
    w, h = int(infos[0].width), int(infos[0].height)
    for i, r in enumerate(infos):
        if (int(r.width), int(r.height)) != (w, h):
            raise ValueError(f"file {i} is {int(r.width)} x {int(r.height)}, file 0 is {w} x {h}: one batch tensor takes one size")
    n = len(infos)
    batch = torch.empty((n, channels, h, w) if layout == "NCHW" else (n, h, w, channels), dtype=dtype, device=device)
    infos, _ = png_decode_device_batch(files, outs=png_sinks(batch, layout, "RGBA", bitdepth), lib=lib)
    return infos, batch


def _png_are_sources(images):
    """Whether a list holds PngSources (all of it: a mixed list is an error)."""
    kinds = {isinstance(image, PngSource) and not isinstance(image, PngSink) for image in images}
    if kinds == {True, False}:
        raise ValueError("a list holds PngSources or images, not both")
    return kinds == {True}


def _png_source_array(sources):
    n = len(sources)
    return (PngSourceStruct * max(n, 1))(*[s.struct for s in sources])


# png_encode_* and png_optimize_* differ in the symbols they call: `name` for images, `source_name` for PngSources.
def _png_one(name, source_name, image, strategy, options, predefined, lib, lossy):
    if isinstance(image, PngSource):
        types = _png_types(predefined, image.height)
        _sync_torch([image.tensor])
        return _png_single(source_name, PngSourceStruct, image.struct, strategy, options, types, lib, lossy)
    im = _png_image(image)
    return _png_single(name, PngImage, im, strategy, options, _png_types(predefined, im.height), lib, lossy, suffixed=True)


def _png_one_out(name, source_name, image, dst, strategy, options, predefined, lib, lossy):
    if isinstance(image, PngSource):
        types = _png_types(predefined, image.height)
        _sync_torch([image.tensor])
        return _png_single_out(source_name, PngSourceStruct, image.struct, dst, strategy, options, types, lib, lossy)
    im = _png_image(image)
    return _png_single_out(name, PngImage, im, dst, strategy, options, _png_types(predefined, im.height), lib, lossy)


def _png_structs(images):
    """(whether they are PngSources, the struct type, the structs) of a list of images or of PngSources; the current stream
    of every torch device among their tensors is synchronised once."""
    if _png_are_sources(images):
        _sync_torch(s.tensor for s in images)
        return True, PngSourceStruct, [s.struct for s in images]
    ims = [_png_image(image, sync=False) for image in images]
    _sync_torch(images)
    return False, PngImage, ims


def _png_many(name, source_name, images, strategy, options, lib, lossy):
    sources, struct, ims = _png_structs(images)
    return _png_batch(source_name if sources else name, struct, ims, strategy, options, lib, lossy, suffixed=not sources)


def png_source_image(source, lib=None):
    """zmx_png_source_image: (width, height, colortype, bitdepth, bytes) of the packed image of a PngSource — host
    arithmetic; RuntimeError for a source the entries refuse without asking the runtime about its memory."""
    lib = lib or library()
    im, nbytes = PngImage(), ctypes.c_size_t(0)
    fn = lib.zmx_png_source_image
    fn.argtypes = [ctypes.POINTER(PngSourceStruct), ctypes.POINTER(PngImage), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(source.struct), ctypes.byref(im), ctypes.byref(nbytes)) != 0:
        raise RuntimeError((lib.zmx_last_error() or b"").decode())
    return int(im.width), int(im.height), int(im.colortype), int(im.bitdepth), int(nbytes.value)


def png_encode_device(image, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, lossy_8bit=False):
    """zmx_png_encode_device: the image in device memory as the PNG file `zopflipng --keepcolortype --always_zopflify
    --filters=<strategy>` writes for it (when options.numiterations is zopflipng's: 15 below 200 000 bytes of scanlines,
    else 5).  `image`: a contiguous uint8 tensor (H, W) grey, (H, W, 2) grey + alpha, (H, W, 3) RGB or (H, W, 4) RGBA — a
    torch tensor's current stream is synchronised first — or (pointer, width, height, colortype, bitdepth) for any of
    the colour types 0, 2, 4, 6 at 8 or 16 bits (16-bit samples big-endian).  `strategy`: one of "0" "1" "2" "3" "4" "m"
    "e" "b", "p" with `predefined`, a filter type (0 .. 4) for every row, or "auto" (PNG_FILTER_AUTO): zopflipng's own
    choice, the file it writes without --filters (`predefined`, where given, is the eighth trial).  `lossy_transparent`, `lossy_8bit`: zopflipng's
    --lossy_transparent and --lossy_8bit (zmx_png_encode_device_lossy; under --keepcolortype the second does nothing and
    the first nothing to a 16-bit image).  Returns the file's bytes.  Raises ValueError for a tensor that is no image,
    RuntimeError with the library's message when the library refuses or fails.
    `image` may also be a PngSource — a strided, planar, float or 16-bit tensor as it lies (zmx_png_encode_source_device):
    the file is the one its packed image gives."""
    return _png_one("zmx_png_encode_device", "zmx_png_encode_source_device", image, strategy, options, predefined, lib,
                    _png_lossy(lossy_transparent, lossy_8bit))


def png_encode_device_batch(images, strategy="e", options=None, lib=None, lossy_transparent=False, lossy_8bit=False):
    """zmx_png_encode_device_batch: one PNG file per image, each the one png_encode_device gives, from one call that
    shares its deflate work among them.  `images`: a list of what png_encode_device takes (the current stream of every
    torch device among the tensors is synchronised once).  Predefined types are the single call's.  A list of PngSources
    (png_sources gives one for a batch tensor) goes to zmx_png_encode_source_device_batch: one launch packs them all."""
    return _png_many("zmx_png_encode_device_batch", "zmx_png_encode_source_device_batch", images, strategy, options, lib,
                     _png_lossy(lossy_transparent, lossy_8bit))


class PngColorStats(ctypes.Structure):
    """zmx_png_color_stats; `colors()` the palette's numcolors entries (r, g, b, a), none for 0 and 257."""
    _fields_ = [("colored", ctypes.c_uint32), ("key", ctypes.c_uint32), ("alpha", ctypes.c_uint32), ("numcolors", ctypes.c_uint32),
                ("bits", ctypes.c_uint32), ("key_r", ctypes.c_uint16), ("key_g", ctypes.c_uint16), ("key_b", ctypes.c_uint16),
                ("reserved", ctypes.c_uint16), ("palette", ctypes.c_ubyte * 1024)]

    def colors(self):
        n = self.numcolors if self.numcolors <= 256 else 0
        return [tuple(self.palette[4 * i:4 * i + 4]) for i in range(n)]


class PngColorMode(ctypes.Structure):
    """zmx_png_color_mode; `colors()` the palettesize entries (r, g, b, a)."""
    _fields_ = [("colortype", ctypes.c_uint32), ("bitdepth", ctypes.c_uint32), ("palettesize", ctypes.c_uint32),
                ("key_defined", ctypes.c_uint32), ("key_r", ctypes.c_uint16), ("key_g", ctypes.c_uint16), ("key_b", ctypes.c_uint16),
                ("reserved", ctypes.c_uint16), ("palette", ctypes.c_ubyte * 1024)]

    def colors(self):
        return [tuple(self.palette[4 * i:4 * i + 4]) for i in range(min(self.palettesize, 256))]


def png_choose_color(stats, numpixels, lib=None):
    """zmx_png_choose_color: the colour mode LodePNG takes for these statistics (a PngColorStats) of an image of
    `numpixels` pixels: a PngColorMode.  Host arithmetic only."""
    lib = lib or library()
    mode = PngColorMode()
    fn = lib.zmx_png_choose_color
    fn.argtypes = [ctypes.POINTER(PngColorStats), ctypes.c_uint64, ctypes.POINTER(PngColorMode)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(stats), int(numpixels), ctypes.byref(mode)) != 0:
        raise RuntimeError("zmx_png_choose_color: " + (lib.zmx_last_error() or b"").decode())
    return mode


def png_optimize_device(image, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, lossy_8bit=False):
    """zmx_png_optimize_device: png_encode_device with the colour mode reduced first — the file `zopflipng
    --always_zopflify --filters=<strategy>` (no --keepcolortype) writes for the image: grey, a palette, a key or fewer
    bits where the pixels allow it, and RGB or RGBA instead of a palette where that makes a small file smaller.
    `lossy_8bit` encodes a 16-bit image as the 8-bit image of its high bytes, `lossy_transparent` gives the pixels with
    alpha 0 of an image that is 8-bit by then the RGB zopflipng gives them (zmx_png_optimize_device_lossy).  Arguments,
    result and errors as png_encode_device's, a PngSource included (zmx_png_optimize_source_device)."""
    return _png_one("zmx_png_optimize_device", "zmx_png_optimize_source_device", image, strategy, options, predefined, lib,
                    _png_lossy(lossy_transparent, lossy_8bit))


def png_optimize_device_batch(images, strategy="e", options=None, lib=None, lossy_transparent=False, lossy_8bit=False):
    """zmx_png_optimize_device_batch: one file per image, each the one png_optimize_device gives, from one call.
    Arguments as png_encode_device_batch's, a list of PngSources included (zmx_png_optimize_source_device_batch)."""
    return _png_many("zmx_png_optimize_device_batch", "zmx_png_optimize_source_device_batch", images, strategy, options, lib,
                     _png_lossy(lossy_transparent, lossy_8bit))


def png_bound(width, height=None, colortype=None, bitdepth=None, lib=None):
    """zmx_png_bound: a destination capacity that does for png_encode_device_out and png_optimize_device_out of any image
    of this width, height, colour type and bit depth (0 for a mode the entries refuse).  png_bound(source) of a PngSource:
    zmx_png_source_bound, the bound of its packed image's mode."""
    lib = lib or library()
    if isinstance(width, PngSource):
        fn = lib.zmx_png_source_bound
        fn.argtypes = [ctypes.POINTER(PngSourceStruct)]
        fn.restype = ctypes.c_size_t
        return int(fn(ctypes.byref(width.struct)))
    fn = lib.zmx_png_bound
    fn.argtypes = [ctypes.c_uint32] * 4
    fn.restype = ctypes.c_size_t
    return int(fn(int(width), int(height), int(colortype), int(bitdepth)))


def png_batch_bound(images, align=1, lib=None):
    """zmx_png_batch_bound: an arena capacity that does for png_encode_device_batch_packed of these images (what
    png_encode_device takes, or bare (None, width, height, colortype, bitdepth) tuples: the pixels are not looked at), or of
    these PngSources (zmx_png_source_batch_bound)."""
    lib = lib or library()
    if _png_are_sources(images):
        fn = lib.zmx_png_source_batch_bound
        fn.argtypes = [ctypes.c_size_t, ctypes.POINTER(PngSourceStruct), ctypes.c_size_t]
        fn.restype = ctypes.c_size_t
        return int(fn(len(images), _png_source_array(images), int(align)))
    ims = [_png_image(image, sync=False) for image in images]
    n = len(ims)
    fn = lib.zmx_png_batch_bound
    fn.argtypes = [ctypes.c_size_t, ctypes.POINTER(PngImage), ctypes.c_size_t]
    fn.restype = ctypes.c_size_t
    return int(fn(n, (PngImage * max(n, 1))(*ims), int(align)))


def png_encode_device_out(image, dst, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, lossy_8bit=False):
    """zmx_png_encode_device_to_device: png_encode_device's file left in device memory.  `dst`: a contiguous tensor or an
    (integer device pointer, capacity) pair on the image's device, of any byte alignment.  Returns the file's size: its
    bytes are dst[0, size), and no byte behind them is written.  Raises CapacityError (with the size needed, nothing
    written) when the file does not fit — png_bound gives a capacity that always does —, otherwise as png_encode_device.
    A PngSource goes to zmx_png_encode_source_device_to_device; `dst` may not overlap the bytes its samples span."""
    return _png_one_out("zmx_png_encode_device_to_device", "zmx_png_encode_source_device_to_device", image, dst, strategy, options,
                        predefined, lib, _png_lossy(lossy_transparent, lossy_8bit))


def png_optimize_device_out(image, dst, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, lossy_8bit=False):
    """zmx_png_optimize_device_to_device: png_optimize_device's file left in device memory; arguments, result and errors as
    png_encode_device_out's (a PngSource: zmx_png_optimize_source_device_to_device)."""
    return _png_one_out("zmx_png_optimize_device_to_device", "zmx_png_optimize_source_device_to_device", image, dst, strategy, options,
                        predefined, lib, _png_lossy(lossy_transparent, lossy_8bit))


def png_encode_device_batch_packed(images, arena, align=1, strategy="e", options=None, lib=None, lossy_transparent=False, lossy_8bit=False):
    """zmx_png_encode_device_batch_packed: png_encode_device_batch's files packed into `arena`, a contiguous tensor or an
    (integer device pointer, capacity) pair: file i begins at the end of file i - 1 rounded up to `align` (a power of two,
    1 .. 4096); the bytes between files are not written.  Returns (offsets, sizes).  Raises CapacityError (`needed`: the
    list of sizes, nothing written) when the arena is too small — png_batch_bound gives one that does.  A list of PngSources
    goes to zmx_png_encode_source_device_batch_packed."""
    sources, struct, ims = _png_structs(images)
    name = "zmx_png_encode_source_device_batch_packed" if sources else "zmx_png_encode_device_batch_packed"
    return _png_batch_packed(name, struct, ims, arena, align, strategy, options, lib, _png_lossy(lossy_transparent, lossy_8bit))


class PngIndexImage(ctypes.Structure):
    """zmx_png_index_image"""
    _fields_ = [("d_pixels", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("colortype", ctypes.c_uint32),
                ("bitdepth", ctypes.c_uint32), ("palettesize", ctypes.c_uint32), ("palette", ctypes.c_ubyte * 1024)]


def _png_index_image(image, palette=None, bitdepth=8, sync=True):
    """The zmx_png_index_image of (tensor or pointer, width, height, colortype, bitdepth, palette) — rows of
    (width * bitdepth + 7) // 8 bytes, colour type 3 with a palette or 0 (grey at 1, 2, 4 bits; palette None) — or of a
    2-D uint8 CUDA tensor of indices with `palette` and bitdepth 8.  A palette is n x 4 (r, g, b, a) or n x 3 (opaque)
    uint8 values, anything numpy.asarray takes."""
    import numpy as np
    if isinstance(image, (tuple, list)):
        src, width, height, colortype, bitdepth, palette = image
        ptr = int(src) if isinstance(src, int) else _device_range(src, None, sync=sync)[0]
    else:
        shape = tuple(image.shape)
        if len(shape) != 2 or image.element_size() != 1 or int(bitdepth) != 8:
            raise ValueError("an index tensor is uint8 of shape (H, W) at 8 bits; packed rows go as "
                             "(tensor_or_pointer, width, height, colortype, bitdepth, palette)")
        ptr, _ = _device_range(image, None, sync=sync)
        height, width, colortype = shape[0], shape[1], 3
    im = PngIndexImage(ptr or None, int(width), int(height), int(colortype), int(bitdepth), 0)
    if palette is not None:
        pal = np.asarray(palette, dtype=np.uint8)
        if pal.ndim != 2 or pal.shape[1] not in (3, 4) or pal.shape[0] > 256:
            raise ValueError("a palette is at most 256 rows of r, g, b, a or r, g, b")
        if pal.shape[1] == 3:
            pal = np.concatenate([pal, np.full((pal.shape[0], 1), 255, dtype=np.uint8)], axis=1)
        im.palettesize = pal.shape[0]
        ctypes.memmove(im.palette, np.ascontiguousarray(pal).ctypes.data, 4 * pal.shape[0])
    elif int(colortype) == 3:
        raise ValueError("a palette image needs its palette")
    return im


def _png_index_single(name, image, strategy, options, predefined, lib, lossy_transparent, palette, bitdepth):
    im = _png_index_image(image, palette, bitdepth)
    return _png_single(name, PngIndexImage, im, strategy, options, _png_types(predefined, im.height), lib, _png_lossy(lossy_transparent, False))


def png_index_encode_device(image, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, palette=None, bitdepth=8):
    """zmx_png_index_encode_device: a palette, 1/2/4-bit grey or index image in device memory — a label map with its colour
    map, a mask, an atlas — as the PNG file `zopflipng --keepcolortype --always_zopflify --filters=<strategy>
    [--lossy_transparent]` writes for it: the input's colour type, depth and palette, in the input's order.  `image`:
    (tensor or pointer, width, height, colortype, bitdepth, palette) with rows of (width * bitdepth + 7) // 8 bytes, the
    first pixel in a byte's top bits — colour type 3 at 1, 2, 4, 8 bits with a palette of n x 4 or n x 3 uint8 values, or
    colour type 0 at 1, 2, 4 bits with palette None — or a 2-D uint8 CUDA tensor of indices with `palette=` and
    `bitdepth=8`.  `strategy`, `predefined`, result and errors as png_encode_device's."""
    return _png_index_single("zmx_png_index_encode_device", image, strategy, options, predefined, lib, lossy_transparent, palette, bitdepth)


def png_index_optimize_device(image, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, palette=None, bitdepth=8):
    """zmx_png_index_optimize_device: the same without --keepcolortype — byte for byte png_optimize_device's file of the
    image expanded to RGBA8, with no expansion made.  Arguments as png_index_encode_device's."""
    return _png_index_single("zmx_png_index_optimize_device", image, strategy, options, predefined, lib, lossy_transparent, palette, bitdepth)


def _png_index_out(name, image, dst, strategy, options, predefined, lib, lossy_transparent, palette, bitdepth):
    im = _png_index_image(image, palette, bitdepth)
    return _png_single_out(name, PngIndexImage, im, dst, strategy, options, _png_types(predefined, im.height), lib,
                           _png_lossy(lossy_transparent, False))


def png_index_encode_device_out(image, dst, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, palette=None,
                                bitdepth=8):
    """zmx_png_index_encode_device_to_device: png_index_encode_device's file left in device memory; `dst`, result and
    errors as png_encode_device_out's — png_index_bound gives a capacity that always does."""
    return _png_index_out("zmx_png_index_encode_device_to_device", image, dst, strategy, options, predefined, lib, lossy_transparent, palette,
                          bitdepth)


def png_index_optimize_device_out(image, dst, strategy="e", options=None, predefined=None, lib=None, lossy_transparent=False, palette=None,
                                  bitdepth=8):
    """zmx_png_index_optimize_device_to_device: png_index_optimize_device's file left in device memory."""
    return _png_index_out("zmx_png_index_optimize_device_to_device", image, dst, strategy, options, predefined, lib, lossy_transparent, palette,
                          bitdepth)


def _png_index_batch(name, images, strategy, options, lib, lossy_transparent):
    ims = [_png_index_image(image, sync=False) for image in images]
    _sync_torch(image[0] if isinstance(image, (tuple, list)) else image for image in images)
    return _png_batch(name, PngIndexImage, ims, strategy, options, lib, _png_lossy(lossy_transparent, False))


def png_index_encode_device_batch(images, strategy="e", options=None, lib=None, lossy_transparent=False):
    """zmx_png_index_encode_device_batch: one file per image, each the one png_index_encode_device gives, from one call
    that shares its deflate work among them.  `images`: a list of (tensor or pointer, width, height, colortype, bitdepth,
    palette) tuples.  Predefined types are the single call's."""
    return _png_index_batch("zmx_png_index_encode_device_batch", images, strategy, options, lib, lossy_transparent)


def png_index_optimize_device_batch(images, strategy="e", options=None, lib=None, lossy_transparent=False):
    """zmx_png_index_optimize_device_batch: one file per image, each the one png_index_optimize_device gives."""
    return _png_index_batch("zmx_png_index_optimize_device_batch", images, strategy, options, lib, lossy_transparent)


def png_index_bound(width, height, colortype, bitdepth, lib=None):
    """zmx_png_index_bound: a destination capacity that does for png_index_encode_device_out and
    png_index_optimize_device_out of any such image (0 for one the entries refuse)."""
    lib = lib or library()
    fn = lib.zmx_png_index_bound
    fn.argtypes = [ctypes.c_uint32] * 4
    fn.restype = ctypes.c_size_t
    return int(fn(int(width), int(height), int(colortype), int(bitdepth)))


def _png_first(first):
    return (ctypes.c_uint64 * 256)(*[int(f) for f in first])


def png_index_color_stats(image, first, lossy_transparent=False, lib=None):
    """zmx_png_index_color_stats: the PngColorStats of the image's RGBA8 expansion (after --lossy_transparent where asked)
    from its first-appearance table (Context.png_index_use_device).  Host arithmetic only; the pixels are not looked at."""
    lib = lib or library()
    im = _png_index_image(image, sync=False) if isinstance(image, (tuple, list)) else image
    stats = PngColorStats()
    fn = lib.zmx_png_index_color_stats
    fn.argtypes = [ctypes.POINTER(PngIndexImage), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint, ctypes.POINTER(PngColorStats)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(im), _png_first(first), _png_lossy(lossy_transparent, False), ctypes.byref(stats)) != 0:
        raise RuntimeError("zmx_png_index_color_stats: " + (lib.zmx_last_error() or b"").decode())
    return stats


def png_index_table(image, first, mode, lossy_transparent=False, lib=None):
    """zmx_png_index_table: the 256 entries that take the image into `mode` (a PngColorMode), for
    Context.png_index_convert_device.  Host arithmetic only."""
    lib = lib or library()
    im = _png_index_image(image, sync=False) if isinstance(image, (tuple, list)) else image
    table = (ctypes.c_uint32 * 256)()
    fn = lib.zmx_png_index_table
    fn.argtypes = [ctypes.POINTER(PngIndexImage), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint, ctypes.POINTER(PngColorMode),
                   ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(im), _png_first(first), _png_lossy(lossy_transparent, False), ctypes.byref(mode), table) != 0:
        raise RuntimeError("zmx_png_index_table: " + (lib.zmx_last_error() or b"").decode())
    return [int(v) for v in table]


def png_index_keep_plan(image, first, lossy_transparent=False, lib=None):
    """zmx_png_index_keep_plan: (the PngColorMode of the --keepcolortype file, the table into it).  Host arithmetic only."""
    lib = lib or library()
    im = _png_index_image(image, sync=False) if isinstance(image, (tuple, list)) else image
    mode = PngColorMode()
    table = (ctypes.c_uint32 * 256)()
    fn = lib.zmx_png_index_keep_plan
    fn.argtypes = [ctypes.POINTER(PngIndexImage), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint, ctypes.POINTER(PngColorMode),
                   ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
    if fn(ctypes.byref(im), _png_first(first), _png_lossy(lossy_transparent, False), ctypes.byref(mode), table) != 0:
        raise RuntimeError("zmx_png_index_keep_plan: " + (lib.zmx_last_error() or b"").decode())
    return mode, [int(v) for v in table]


def last_output_traffic(lib=None):
    """zmx_last_output_traffic: of this thread's last call, the stream's bytes device to host, its bytes host to device,
    the blocks whose symbols' bits never left the device, the blocks the host wrote and uploaded."""
    lib = lib or library()
    t = (ctypes.c_double * 4)()
    fn = lib.zmx_last_output_traffic
    fn.argtypes = [ctypes.POINTER(ctypes.c_double)]
    fn.restype = ctypes.c_int
    fn(t)
    return [float(v) for v in t]


def last_input_traffic(lib=None):
    """zmx_last_input_traffic: input bytes of this thread's last call that went host to device, device to device,
    device to host."""
    lib = lib or library()
    t = (ctypes.c_double * 3)()
    fn = lib.zmx_last_input_traffic
    fn.argtypes = [ctypes.POINTER(ctypes.c_double)]
    fn.restype = ctypes.c_int
    fn(t)
    return [float(v) for v in t]


def deflate(data, btype=2, final=1, options=None, lib=None):
    """ZopfliDeflate (deflate.c:908) from bp = 0; returns (bytes, bp)."""
    lib = lib or library()
    options = options or ZopfliOptions()
    out, size, bp = _u8p(), ctypes.c_size_t(0), ctypes.c_ubyte(0)
    lib.ZopfliDeflate(ctypes.byref(options), btype, final, data, len(data), ctypes.byref(bp), ctypes.byref(out),
                      ctypes.byref(size))
    return _take(out, size), bp.value


def deflate_part(data, instart, inend, btype=2, final=1, options=None, lib=None):
    """ZopfliDeflatePart (deflate.c:811) from bp = 0; returns (bytes, bp)."""
    lib = lib or library()
    options = options or ZopfliOptions()
    out, size, bp = _u8p(), ctypes.c_size_t(0), ctypes.c_ubyte(0)
    lib.ZopfliDeflatePart(ctypes.byref(options), btype, final, data, instart, inend, ctypes.byref(bp),
                          ctypes.byref(out), ctypes.byref(size))
    return _take(out, size), bp.value


def last_timing(lib=None):
    lib = lib or library()
    t = (ctypes.c_double * 8)()
    lib.zmx_last_timing(t)
    keys = ["tables", "greedy", "squeeze", "cost_model", "split", "encode", "dp_kernel", "squeeze_launches"]
    d = dict(zip(keys, list(t)))
    k = (ctypes.c_double * 4)()
    lib.zmx_last_kernel_timing(k)
    d["wtab_kernel"], d["trace_kernel"] = k[0], k[2]
    h = (ctypes.c_double * 2)()
    lib.zmx_last_host_timing(h)
    d["download"], d["serialize"] = h[0], h[1]
    m = (ctypes.c_double * 4)()
    lib.zmx_last_match_timing(m)
    d["match_kernel"], d["hash_kernels"], d["table_builds"], d["positions_matched"] = m[0], m[1], m[2], m[3]
    w = (ctypes.c_double * 3)()
    lib.zmx_last_match_walk(w)
    d["skip_walk_lane_iterations"], d["skip_walk_wave_iterations"], d["skip_walk_positions"] = w[0], w[1], w[2]
    return d


# the slots of zmx_last_seg_stats, in the order of enum zmx_seg_stat (csrc/host/zmx_internal.h, the host's reading)
SEG_STAT_KEYS = ["tasks", "accepted", "rerun_state", "rerun_level", "rerun_tie", "positions_rerun", "rerun_values", "positions"]


def last_seg_stats(lib=None):
    """zmx_last_seg_stats: how the chain's tasks of the last call fared."""
    lib = lib or library()
    t = (ctypes.c_double * len(SEG_STAT_KEYS))()
    lib.zmx_last_seg_stats(t)
    return dict(zip(SEG_STAT_KEYS, list(t)))


class Context:
    """The zmx_* device layer: one HIP device with a resident input."""

    def __init__(self, device=0, lib=None):
        self.lib = lib or library()
        self.handle = ctypes.c_void_p()
        self._input = None
        self._nbytes = 0
        self._segments = None
        if self.lib.zmx_ctx_create(device, ctypes.byref(self.handle)) != 0:
            raise RuntimeError("zmx_ctx_create: " + self.error())

    def error(self):
        return (self.lib.zmx_last_error() or b"").decode()

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.error()}")

    def close(self):
        if self.handle:
            self.lib.zmx_ctx_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def pool_stats(self):
        """zmx_internal_pool_stats: the context's memory pool in numbers (reads only).  live / live_bytes: device arrays
        in use; cached / cached_bytes: blocks kept for the next request; device_cached: what all contexts of the device
        keep cached; pinned: cached pinned host buffers; fresh / from_cache: allocations served by hipMalloc / from the
        cache since the context was created."""
        out = (ctypes.c_uint64 * 8)()
        fn = self.lib.zmx_internal_pool_stats
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        fn.restype = None
        fn(self.handle, out)
        keys = ["live", "live_bytes", "cached", "cached_bytes", "device_cached", "pinned", "fresh", "from_cache"]
        return dict(zip(keys, [int(v) for v in out]))

    def trim_cache(self):
        """zmx_ctx_trim_cache: the cached blocks go back to the device."""
        fn = self.lib.zmx_ctx_trim_cache
        fn.argtypes = [ctypes.c_void_p]
        self._check(fn(self.handle), "zmx_ctx_trim_cache")

    def set_input(self, data):
        self._input = data
        self._nbytes = len(data)
        self._segments = None
        self._check(self.lib.zmx_set_input(self.handle, data, len(data)), "zmx_set_input")

    def set_input_device(self, ptr, nbytes):
        """zmx_set_input_device: `nbytes` bytes of device memory at the integer pointer `ptr` become the resident
        input (copied; the buffer may be reused when the call returns)."""
        self._input = None
        self._nbytes = int(nbytes)
        self._segments = None
        fn = self.lib.zmx_set_input_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ptr, nbytes), "zmx_set_input_device")

    def gather_device(self, srcs, dst):
        """zmx_gather_device: the bytes of `srcs` (tensors or (pointer, nbytes) pairs, as compress_device_batch takes
        them) end to end at `dst`, a tensor or an integer pointer into memory of this context's device."""
        ptrs, sizes = _device_ranges(srcs)
        n = len(ptrs)
        if not isinstance(dst, int):
            dst = _device_range(dst, None)[0]
        fn = self.lib.zmx_gather_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                       ctypes.c_void_p]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, n, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_size_t * max(n, 1))(*sizes), dst),
                    "zmx_gather_device")

    def png_filter_types_device(self, image, linebytes, height, bytewidth, strategy, types, windowsize=32768):
        """zmx_png_filter_types_device: the filter type of every row of the image at `image` (a tensor or an integer
        pointer: `height` rows of `linebytes` bytes in memory of this context's device) under `strategy` (a letter of
        zopflipng's --filters= or a ZMX_PNG_FILTER_* number; `windowsize` for "b"), into the `height` bytes at `types`,
        a tensor or an integer pointer into the same device's memory."""
        img = image if isinstance(image, int) else _device_range(image, None)[0]
        dst = types if isinstance(types, int) else _device_range(types, None)[0]
        fn = self.lib.zmx_png_filter_types_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                       ctypes.c_uint, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, img or None, linebytes, height, bytewidth, _png_strategy(strategy), windowsize, dst or None),
                    "zmx_png_filter_types_device")

    def png_filter_rows_device(self, image, linebytes, height, bytewidth, types, out, capacity=None):
        """zmx_png_filter_rows_device: the filtered scanlines of the image at `image` — row r is types[r] and then the
        row filtered that way — into `out`, a tensor or an integer pointer with `capacity` bytes (an integer pointer
        without one: exactly height * (linebytes + 1)); all three in memory of this context's device."""
        img = image if isinstance(image, int) else _device_range(image, None)[0]
        typ = types if isinstance(types, int) else _device_range(types, None)[0]
        if isinstance(out, int):
            dst, capacity = out, height * (linebytes + 1) if capacity is None else int(capacity)
        else:
            dst, capacity = _device_range(out, capacity)
        fn = self.lib.zmx_png_filter_rows_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                       ctypes.c_void_p, ctypes.c_size_t]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, img or None, linebytes, height, bytewidth, typ or None, dst or None, capacity),
                    "zmx_png_filter_rows_device")

    def png_deflate_sizes_device(self, bufs, windowsize=8192):
        """zmx_png_deflate_sizes_device: the length LodePNG's own zlib encoder (default settings, window `windowsize`)
        gives for every buffer of `bufs` (tensors or (pointer, nbytes) pairs in memory of this context's device), all
        sized in one pass over the device: a list of integers."""
        ptrs, sizes = _device_ranges(bufs)
        n = len(ptrs)
        out = (ctypes.c_uint64 * max(n, 1))()
        fn = self.lib.zmx_png_deflate_sizes_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint,
                       ctypes.POINTER(ctypes.c_uint64)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, n, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_size_t * max(n, 1))(*sizes), int(windowsize), out),
                    "zmx_png_deflate_sizes_device")
        return [int(out[i]) for i in range(n)]

    def png_lodeflate_arrays(self, bufs, windowsize=8192, tile_len=0):
        """zmx_internal_png_lodeflate_arrays (a test hook): png_deflate_sizes_device in tiles of `tile_len` positions
        (0: the device's own) together with what its kernels left in device memory: (sizes, HC, ZC, LD, counts) — the
        three per-position arrays over all buffers' positions, one buffer after the other, and the symbol counts as
        [deflate blocks of all buffers][318], numpy uint32."""
        import numpy as np
        ptrs, sizes = _device_ranges(bufs)
        n = len(ptrs)
        positions = sum(sizes)
        nblocks = sum(-(-s // min(262144, max(65536, s // 8 + 8))) for s in sizes)      # lodepng_deflatev's blocks
        hc, zc, ld = (np.zeros(max(positions, 1), dtype=np.uint32) for _ in range(3))
        counts = np.zeros((max(nblocks, 1), 318), dtype=np.uint32)
        out = (ctypes.c_uint64 * max(n, 1))()
        fn = self.lib.zmx_internal_png_lodeflate_arrays
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint,
                       ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, n, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_size_t * max(n, 1))(*sizes), int(windowsize),
                       int(tile_len), hc.ctypes.data, zc.ctypes.data, ld.ctypes.data, counts.ctypes.data, out),
                    "zmx_internal_png_lodeflate_arrays")
        return [int(out[i]) for i in range(n)], hc[:positions], zc[:positions], ld[:positions], counts[:nblocks]

    def png_brute_sizes(self, image, linebytes, height, bytewidth, windowsize=32768, force_scratch=False, max_workgroups=0):
        """zmx_internal_png_brute_sizes (a test hook): zmx_png_filter_types_brute of the host image `image` (bytes or a
        uint8 array: `height` rows of `linebytes` bytes) together with what k_png_brute computed: (sizes, bits, types) —
        sizes and bits as numpy uint64 [height][5], the zlib bytes and the fixed-code bit count of every row under
        every filter type; types numpy uint8 [height].  `force_scratch` keeps the kernel's per-position arrays out of
        the LDS whatever the row length; `max_workgroups` caps the grid (0: the driver's own choice)."""
        import numpy as np
        raw = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray)) else image, dtype=np.uint8)
        if raw.size != linebytes * height:
            raise ValueError(f"{raw.size} bytes for {height} rows of {linebytes}")
        sizes = np.zeros((max(height, 1), 5), dtype=np.uint64)
        bits = np.zeros((max(height, 1), 5), dtype=np.uint64)
        types = np.full(max(height, 1), 255, dtype=np.uint8)
        fn = self.lib.zmx_internal_png_brute_sizes
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int,
                       ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, raw.ctypes.data, linebytes, height, bytewidth, int(windowsize), 1 if force_scratch else 0,
                       int(max_workgroups), sizes.ctypes.data, bits.ctypes.data, types.ctypes.data), "zmx_internal_png_brute_sizes")
        return sizes[:height], bits[:height], types[:height]

    def png_choose_strategy_device(self, image, reduce_color=False, predefined=None):
        """zmx_png_choose_strategy_device: zopflipng's choice of the filter strategy for the image (`image` as
        png_encode_device takes it; `reduce_color`: without --keepcolortype; `predefined`: a type per row for the eighth
        trial): (the ZMX_PNG_FILTER_* number, the eight trial file sizes, 0 for a trial that was not run)."""
        im = _png_image(image)
        types = None if predefined is None else bytes(bytearray(int(t) for t in predefined))
        if types is not None and len(types) != im.height:
            raise ValueError(f"{len(types)} predefined types for {im.height} rows")
        strategy = ctypes.c_int(-1)
        sizes = (ctypes.c_uint64 * 8)()
        fn = self.lib.zmx_png_choose_strategy_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(PngImage), ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                       ctypes.POINTER(ctypes.c_uint64)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ctypes.byref(im), 1 if reduce_color else 0, types, ctypes.byref(strategy), sizes),
                    "zmx_png_choose_strategy_device")
        return int(strategy.value), [int(v) for v in sizes]

    def png_color_stats_device(self, image):
        """zmx_png_color_stats_device: LodePNG's colour statistics of an image in memory of this context's device
        (`image` as png_encode_device takes it): a PngColorStats."""
        im = _png_image(image)
        stats = PngColorStats()
        fn = self.lib.zmx_png_color_stats_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(PngImage), ctypes.POINTER(PngColorStats)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ctypes.byref(im), ctypes.byref(stats)), "zmx_png_color_stats_device")
        return stats

    def png_convert_device(self, image, mode, out, capacity=None):
        """zmx_png_convert_device: the image in the colour mode `mode` (a PngColorMode, png_choose_color's or the caller's)
        into `out`, a tensor or an integer pointer with `capacity` bytes (an integer pointer without one: exactly the
        output's size), memory of this context's device: height rows of (width * bpp + 7) // 8 bytes."""
        im = _png_image(image)
        if isinstance(out, int):
            bpp = (1 if mode.colortype == 3 else {0: 1, 2: 3, 4: 2, 6: 4}.get(mode.colortype, 0)) * mode.bitdepth
            dst, capacity = out, im.height * ((im.width * bpp + 7) // 8) if capacity is None else int(capacity)
        else:
            dst, capacity = _device_range(out, capacity)
        fn = self.lib.zmx_png_convert_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(PngImage), ctypes.POINTER(PngColorMode), ctypes.c_void_p, ctypes.c_size_t]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ctypes.byref(im), ctypes.byref(mode), dst or None, capacity), "zmx_png_convert_device")

    def png_pack_device(self, sources, outs):
        """zmx_png_pack_device: the packed images of `sources` (PngSources: rows back to back, PNG byte order, 16-bit
        samples big-endian) into `outs`, as many contiguous tensors or (integer device pointer, capacity) pairs on this
        context's device, of any byte alignment — ONE launch whatever their number.  The tensors' current streams are
        synchronised once per device."""
        if len(sources) != len(outs):
            raise ValueError(f"{len(sources)} sources, but {len(outs)} destinations")
        _sync_torch(s.tensor for s in sources)
        ptrs, capacities = _device_ranges(outs)
        n = len(sources)
        fn = self.lib.zmx_png_pack_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(PngSourceStruct), ctypes.POINTER(ctypes.c_void_p),
                       ctypes.POINTER(ctypes.c_size_t)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, n, _png_source_array(sources), (ctypes.c_void_p * max(n, 1))(*ptrs),
                       (ctypes.c_size_t * max(n, 1))(*capacities)), "zmx_png_pack_device")

    def png_unpack_device(self, modes, owns, sinks):
        """zmx_png_unpack_device: own-mode pixels into sinks — modes[i] (a PngDecodeResult of png_info_device or of a decode)
        says what owns[i] (a contiguous uint8 tensor or an (integer device pointer, nbytes) pair: the OWN mode's bytes)
        holds, sinks[i] (a PngSink) where it goes.  ONE launch whatever their number.  The tensors' current streams are
        synchronised once per device."""
        if not len(modes) == len(owns) == len(sinks):
            raise ValueError(f"{len(modes)} modes, {len(owns)} images, {len(sinks)} sinks")
        _sync_torch(s.tensor for s in sinks)
        ptrs, _ = _device_ranges(owns)
        n = len(sinks)
        fn = self.lib.zmx_png_unpack_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(PngDecodeResult), ctypes.POINTER(ctypes.c_void_p),
                       ctypes.POINTER(PngSinkStruct)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, n, (PngDecodeResult * max(n, 1))(*modes), (ctypes.c_void_p * max(n, 1))(*ptrs), _png_sink_array(sinks)),
                    "zmx_png_unpack_device")

    def png_lossy_transparent_device(self, image, out, capacity=None):
        """zmx_png_lossy_transparent_device: zopflipng's --lossy_transparent rewrite of the image (`image` as
        png_encode_device takes it) into `out`, a tensor or an integer pointer with `capacity` bytes (an integer pointer
        without one: exactly the image's size), memory of this context's device; `out` may be the image itself.  Returns
        the PngLossyInfo."""
        im = _png_image(image)
        if isinstance(out, int):
            nbytes = im.height * im.width * {0: 1, 2: 3, 4: 2, 6: 4}.get(im.colortype, 0) * (im.bitdepth // 8)
            dst, capacity = out, nbytes if capacity is None else int(capacity)
        else:
            dst, capacity = _device_range(out, capacity)
        info = PngLossyInfo()
        fn = self.lib.zmx_png_lossy_transparent_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(PngImage), ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(PngLossyInfo)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ctypes.byref(im), dst or None, capacity, ctypes.byref(info)), "zmx_png_lossy_transparent_device")
        return info

    def png_index_use_device(self, image, palette=None, bitdepth=8):
        """zmx_png_index_use_device: for each of the 256 values the smallest raster pixel index at which it occurs in the
        index image (`image` as png_index_encode_device takes it), 2**64 - 1 for a value no pixel has: a list of 256."""
        im = _png_index_image(image, palette, bitdepth)
        first = (ctypes.c_uint64 * 256)()
        fn = self.lib.zmx_png_index_use_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(PngIndexImage), ctypes.POINTER(ctypes.c_uint64)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ctypes.byref(im), first), "zmx_png_index_use_device")
        return [int(v) for v in first]

    def png_index_convert_device(self, image, mode, table, out, capacity=None, palette=None, bitdepth=8):
        """zmx_png_index_convert_device: the index image through `table` (256 integers: png_index_table's, png_index_keep_plan's
        or the caller's) into the colour mode `mode` (a PngColorMode), into `out`, a tensor or an integer pointer with
        `capacity` bytes (an integer pointer without one: exactly the output's size), memory of this context's device:
        height rows of (width * bpp + 7) // 8 bytes."""
        im = _png_index_image(image, palette, bitdepth)
        if isinstance(out, int):
            bpp = (1 if mode.colortype == 3 else {0: 1, 2: 3, 4: 2, 6: 4}.get(mode.colortype, 0)) * mode.bitdepth
            dst, capacity = out, im.height * ((im.width * bpp + 7) // 8) if capacity is None else int(capacity)
        else:
            dst, capacity = _device_range(out, capacity)
        fn = self.lib.zmx_png_index_convert_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(PngIndexImage), ctypes.POINTER(PngColorMode), ctypes.POINTER(ctypes.c_uint32),
                       ctypes.c_void_p, ctypes.c_size_t]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ctypes.byref(im), ctypes.byref(mode), (ctypes.c_uint32 * 256)(*[int(v) for v in table]), dst or None,
                       capacity), "zmx_png_index_convert_device")

    def png_index_choose_strategy_device(self, image, reduce_color=False, predefined=None, lossy_transparent=False, palette=None, bitdepth=8):
        """zmx_png_index_choose_strategy_device: png_choose_strategy_device for an index image, --lossy_transparent applied
        first where asked: (the ZMX_PNG_FILTER_* number, the eight trial file sizes)."""
        im = _png_index_image(image, palette, bitdepth)
        types = _png_types(predefined, im.height)
        strategy = ctypes.c_int(-1)
        sizes = (ctypes.c_uint64 * 8)()
        fn = self.lib.zmx_png_index_choose_strategy_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(PngIndexImage), ctypes.c_int, ctypes.c_uint, ctypes.c_char_p,
                       ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, ctypes.byref(im), 1 if reduce_color else 0, _png_lossy(lossy_transparent, False), types,
                       ctypes.byref(strategy), sizes), "zmx_png_index_choose_strategy_device")
        return int(strategy.value), [int(v) for v in sizes]

    def bitjoin_device(self, pieces, total_bits, dst, capacity=None):
        """zmx_bitjoin_device: pieces = [(src pointer, src_bit, nbits, dst_bit)] — bits [src_bit, src_bit + nbits) of the
        bit string at the integer device pointer become bits [dst_bit, dst_bit + nbits) of the one at `dst`, a tensor or
        an integer pointer with `capacity` bytes, memory of this context's device; bits that no piece covers are 0."""
        class Piece(ctypes.Structure):
            _fields_ = [("src", ctypes.c_void_p), ("src_bit", ctypes.c_uint64), ("nbits", ctypes.c_uint64),
                        ("dst_bit", ctypes.c_uint64)]
        n = len(pieces)
        arr = (Piece * max(n, 1))(*[Piece(int(p[0]) if p[0] else None, int(p[1]), int(p[2]), int(p[3])) for p in pieces])
        dst, capacity = _device_range(dst, capacity)
        fn = self.lib.zmx_bitjoin_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, n, ctypes.cast(arr, ctypes.c_void_p) if n else None, int(total_bits), dst, capacity),
                    "zmx_bitjoin_device")

    def bitjoin_many_device(self, dests, pieces, capacities=None):
        """zmx_bitjoin_many_device: dests = [(dst pointer, total_bits, first_piece, npieces)], pieces as bitjoin_device
        takes them with dst_bit counted from the piece's own destination; destination d is made from
        pieces[first_piece : first_piece + npieces].  `capacities`: the room at every destination in bytes (None: exactly
        its (total_bits + 7) // 8).  One launch for all of them."""
        class Piece(ctypes.Structure):
            _fields_ = [("src", ctypes.c_void_p), ("src_bit", ctypes.c_uint64), ("nbits", ctypes.c_uint64),
                        ("dst_bit", ctypes.c_uint64)]

        class Dest(ctypes.Structure):
            _fields_ = [("dst", ctypes.c_void_p), ("total_bits", ctypes.c_uint64), ("first_piece", ctypes.c_uint64),
                        ("npieces", ctypes.c_uint64)]
        n, nd = len(pieces), len(dests)
        parr = (Piece * max(n, 1))(*[Piece(int(p[0]) if p[0] else None, int(p[1]), int(p[2]), int(p[3])) for p in pieces])
        darr = (Dest * max(nd, 1))(*[Dest(int(d[0]) if d[0] else None, int(d[1]), int(d[2]), int(d[3])) for d in dests])
        caps = None if capacities is None else (ctypes.c_size_t * max(nd, 1))(*[int(c) for c in capacities])
        fn = self.lib.zmx_bitjoin_many_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                       ctypes.c_void_p]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, nd, ctypes.cast(darr, ctypes.c_void_p) if nd else None, caps, n,
                       ctypes.cast(parr, ctypes.c_void_p) if n else None), "zmx_bitjoin_many_device")

    def master_block_costs_device(self):
        """zmx_master_block_costs_device: the dealing costs of the resident input's master blocks, counted on the device."""
        import numpy as np
        cost = np.zeros(max(1, (self._nbytes + 999999) // 1000000), dtype=np.float64)
        fn = self.lib.zmx_master_block_costs_device
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_size_t]
        fn.restype = ctypes.c_int
        n = fn(self.handle, cost.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cost.size)
        if n < 0:
            raise RuntimeError("zmx_master_block_costs_device: " + self.error())
        return cost[:n]

    def set_input_segments(self, starts):
        """zmx_set_input_segments: the resident input is the concatenation of independent inputs starting at
        `starts` (starts[0] = 0, non-decreasing); a block's window stops at the start of its own input."""
        n = len(starts)
        arr = (ctypes.c_uint64 * max(n, 1))(*starts)
        fn = self.lib.zmx_set_input_segments
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, arr, n), "zmx_set_input_segments")
        self._segments = list(starts)

    def window_start(self, instart):
        """Where the window of a block starting at `instart` begins: max(start of its segment, instart - 32768)."""
        floor = 0
        if self._segments:
            floor = max(x for x in self._segments if x <= instart)
        return max(floor, instart - 32768)

    def checksums(self, kind, ranges):
        """zmx_checksums: CRC-32 / Adler-32 of every resident range (begin, end), in one launch set."""
        n = len(ranges)
        b = (ctypes.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
        e = (ctypes.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
        v = (ctypes.c_uint32 * max(n, 1))()
        fn = self.lib.zmx_checksums
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64),
                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, kind, n, b, e, v), "zmx_checksums")
        return [int(v[i]) for i in range(n)]

    def checksum_device(self, kind, ranges):
        """zmx_checksum_device: CRC-32 / Adler-32 of every range of device memory of the context's device — contiguous
        tensors or (integer device pointer, nbytes) pairs, at any byte address —, pieces and finish on the device."""
        ptrs, sizes = _device_ranges(ranges)
        n = len(ptrs)
        v = (ctypes.c_uint32 * max(n, 1))()
        fn = self.lib.zmx_checksum_device
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                       ctypes.POINTER(ctypes.c_uint32)]
        fn.restype = ctypes.c_int
        self._check(fn(self.handle, kind, n, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_size_t * max(n, 1))(*sizes), v),
                    "zmx_checksum_device")
        return [int(v[i]) for i in range(n)]

    def inflate_device(self, streams, format="gzip", outs=None):
        """zmx_inflate_device_ctx: the step on this context — k_inflate over `streams` (uint8 tensors or (integer device
        pointer, nbytes) pairs in memory of the context's device) into `outs` (tensors, (pointer, capacity) pairs or None
        entries; None: the size-only mode).  No checksum is compared.  Returns the list of InflateResult, whatever the
        streams' statuses; raises RuntimeError where the call itself is refused or the device fails."""
        return _inflate_call(self.lib, self.lib.zmx_inflate_device_ctx, "zmx_inflate_device_ctx", [self.handle], format, streams, outs)[1]

    def png_decode_device(self, files, mode="rgba8", outs=None, force_wide=False, idat_capacity=None):
        """zmx_png_decode_device_ctx: the decode on this context — `files` (uint8 tensors or (integer device pointer, nbytes)
        pairs in memory of the context's device) into `outs` (tensors, (pointer, capacity) pairs or None entries; None: the
        size-only mode).  Two hooks for tests: `force_wide` sends every image through the wide path (the band carry in
        global memory, a launch a band), `idat_capacity` sets the chunk entries a file has in the first walk.  Returns the
        list of PngDecodeResult, whatever the files' statuses; raises RuntimeError where the call itself is refused or the
        device fails."""
        hooks = PngDecodeHooks(1 if force_wide else 0, int(idat_capacity or 0))
        if outs is not None and _png_are_sinks(outs):
            # (zmx_png_decode_sink_device_ctx: `mode` is ignored)
            return _png_decode_sink_call(self.lib, self.lib.zmx_png_decode_sink_device_ctx, "zmx_png_decode_sink_device_ctx", [self.handle], files,
                                         outs, tail=[(ctypes.POINTER(PngDecodeHooks), ctypes.byref(hooks))])[1]
        return _png_decode_call(self.lib, self.lib.zmx_png_decode_device_ctx, "zmx_png_decode_device_ctx", [self.handle], mode, files, outs,
                                tail=[(ctypes.POINTER(PngDecodeHooks), ctypes.byref(hooks))])[1]

    def build_tables(self, blocks, parent=None, matches_only=False):
        """zmx_tables_build, zmx_tables_build_matches (no DP rows: for the greedy pass and as a parent), or
        zmx_tables_build_from when `parent` (Tables over enclosing blocks) is given."""
        arr = (ZmxBlock * len(blocks))(*[ZmxBlock(s, e) for s, e in blocks])
        t = ctypes.c_void_p()
        if matches_only:
            self._check(self.lib.zmx_tables_build_matches(self.handle, arr, len(blocks), ctypes.byref(t)),
                        "zmx_tables_build_matches")
        elif parent is None:
            self._check(self.lib.zmx_tables_build(self.handle, arr, len(blocks), ctypes.byref(t)), "zmx_tables_build")
        else:
            self._check(self.lib.zmx_tables_build_from(self.handle, parent.handle, arr, len(blocks), ctypes.byref(t)),
                        "zmx_tables_build_from")
        return Tables(self, t, list(blocks))

    def checksum(self, kind, begin, end):
        """zmx_checksum: CRC-32 (kind CRC32) or Adler-32 (ADLER32) of resident bytes [begin, end), on the device."""
        v = ctypes.c_uint32(0)
        self._check(self.lib.zmx_checksum(self.handle, kind, begin, end, ctypes.byref(v)), "zmx_checksum")
        return v.value

    def deflate_range(self, options, instart, inend, final=1, as_array=False):
        """zmx_deflate_range: serialised chunks of ZopfliDeflate over resident bytes [instart, inend).
        as_array=True returns a numpy view of the library's malloc'ed blob (no copy)."""
        blob, size = _u8p(), ctypes.c_size_t(0)
        self._check(self.lib.zmx_deflate_range(self.handle, ctypes.byref(options), instart, inend, final,
                                               ctypes.byref(blob), ctypes.byref(size)), "zmx_deflate_range")
        if as_array:
            return _owned_array(ctypes.cast(blob, ctypes.c_void_p).value, size.value)
        return _take(blob, size)

    def merge(self, blobs, prefix=b"", trailer=b"", as_array=False):
        """zmx_chunks_merge after `prefix` (e.g. a gzip header), then `trailer`: prefix + deflate
        stream + trailer.  Blobs may be bytes or uint8 numpy arrays (not copied); the stream is
        assembled in one malloc'ed buffer (the (out, outsize) convention of the reference, capacity
        = next power of two) and returned as bytes, or as a numpy view of it with as_array=True."""
        import numpy as np
        n = len(blobs)
        keep = [b if isinstance(b, np.ndarray) else np.frombuffer(b, dtype=np.uint8) for b in blobs]
        arr = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
        sizes = (ctypes.c_size_t * n)(*[k.size for k in keep])
        out, size, bp = _u8p(), ctypes.c_size_t(0), ctypes.c_ubyte(0)
        if prefix:
            addr = _libc.malloc(_pow2ceil(len(prefix)))
            ctypes.memmove(addr, prefix, len(prefix))
            out, size = ctypes.cast(addr, _u8p), ctypes.c_size_t(len(prefix))
        self._check(self.lib.zmx_chunks_merge(arr, sizes, n, ctypes.byref(bp), ctypes.byref(out),
                                              ctypes.byref(size)), "zmx_chunks_merge")
        addr, total = ctypes.cast(out, ctypes.c_void_p).value, size.value
        if trailer:
            new = total + len(trailer)
            if addr is None or _pow2ceil(new) > (_pow2ceil(total) if total else 0):
                addr = _libc.realloc(addr, _pow2ceil(new))
            ctypes.memmove(addr + total, trailer, len(trailer))
            total = new
        if as_array:
            return _owned_array(addr, total)
        data = ctypes.string_at(addr, total) if total else b""
        _libc.free(addr)
        return data


class Dist:
    """zmx_dist_*: the ranks' blobs gathered to rank 0 over RCCL by the library itself (one process
    per GPU).  `unique_id()` on rank 0, handed to the others by the launcher, then `Dist(ctx, rank,
    world, id)` on every rank."""

    @staticmethod
    def unique_id(lib=None):
        lib = lib or library()
        buf = ctypes.create_string_buffer(128)
        if lib.zmx_dist_unique_id(buf) != 0:
            raise RuntimeError("zmx_dist_unique_id: " + (lib.zmx_last_error() or b"").decode())
        return buf.raw

    def __init__(self, ctx, rank, world, uid):
        self.ctx, self.rank, self.world = ctx, rank, world
        self.handle = ctypes.c_void_p()
        ctx._check(ctx.lib.zmx_dist_init(ctx.handle, rank, world, uid, ctypes.byref(self.handle)), "zmx_dist_init")

    def gather(self, blob):
        """Returns the list of the ranks' blobs (uint8 arrays, views of one malloc'ed buffer) on rank 0,
        None elsewhere."""
        import numpy as np
        src = blob if isinstance(blob, np.ndarray) else np.frombuffer(blob, dtype=np.uint8)
        out = ctypes.c_void_p()
        sizes = (ctypes.c_size_t * self.world)()
        self.ctx._check(self.ctx.lib.zmx_dist_gather(self.handle, src.ctypes.data if src.size else None, src.size,
                                                     ctypes.byref(out), sizes), "zmx_dist_gather")
        if self.rank != 0:
            return None
        total = sum(sizes)
        whole = _owned_array(out.value, total)
        parts, off = [], 0
        for r in range(self.world):
            parts.append(whole[off:off + sizes[r]])
            off += sizes[r]
        return parts

    def comm_count(self):
        """ncclCommCount of the communicator: the ranks RCCL itself saw."""
        return int(self.ctx.lib.zmx_dist_comm_count(self.handle))

    def close(self):
        if self.handle:
            self.ctx.lib.zmx_dist_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class CostStores:
    """zmx_cost_stores: LZ77 symbol sequences resident on the device with their sampled prefix histograms;
    block_costs = ZopfliCalculateBlockSizeAutoType (deflate.c:610-621) of many ranges at once, on the device."""

    def __init__(self, ctx, handle, sizes):
        self.ctx, self.handle, self.sizes = ctx, handle, list(sizes)

    @staticmethod
    def from_host(ctx, stores):
        """stores = [(litlens, dists)] (lz77.h:44-49 convention)."""
        import numpy as np
        n = len(stores)
        lls = [np.ascontiguousarray(s[0], dtype=np.uint16) for s in stores]
        dds = [np.ascontiguousarray(s[1], dtype=np.uint16) for s in stores]
        pl = (ctypes.c_void_p * n)(*[a.ctypes.data for a in lls])
        pd = (ctypes.c_void_p * n)(*[a.ctypes.data for a in dds])
        ns = (ctypes.c_size_t * n)(*[len(a) for a in lls])
        fn = ctx.lib.zmx_cost_stores_create_host
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        h = ctypes.c_void_p()
        ctx._check(fn(ctx.handle, n, ctypes.cast(pl, ctypes.c_void_p), ctypes.cast(pd, ctypes.c_void_p),
                      ctypes.cast(ns, ctypes.c_void_p), ctypes.byref(h)), "zmx_cost_stores_create_host")
        return CostStores(ctx, h, [len(a) for a in lls])

    @staticmethod
    def from_tables(tables, sequences):
        """sequences = [[(block, slot, nsym), ...], ...]: every sequence the concatenation of device stores of `tables`."""
        ctx = tables.ctx
        first, blk, slot, nsym = [0], [], [], []
        for seq in sequences:
            for b, s, k in seq:
                blk.append(int(b)); slot.append(int(s)); nsym.append(int(k))
            first.append(len(blk))
        n, np_ = len(sequences), len(blk)
        fn = ctx.lib.zmx_cost_stores_create
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_void_p, ctypes.c_void_p]
        a_first = (ctypes.c_size_t * (n + 1))(*first)
        a_blk = (ctypes.c_size_t * max(np_, 1))(*blk)
        a_slot = (ctypes.c_int32 * max(np_, 1))(*slot)
        a_nsym = (ctypes.c_size_t * max(np_, 1))(*nsym)
        h = ctypes.c_void_p()
        ctx._check(fn(ctx.handle, tables.handle, n, ctypes.cast(a_first, ctypes.c_void_p), ctypes.cast(a_blk, ctypes.c_void_p),
                      ctypes.cast(a_slot, ctypes.c_void_p), ctypes.cast(a_nsym, ctypes.c_void_p), ctypes.byref(h)),
                   "zmx_cost_stores_create")
        return CostStores(ctx, h, [sum(k for _, _, k in seq) for seq in sequences])

    def block_costs(self, ranges):
        """ranges = [(sequence, lstart, lend)] -> float64 array of block sizes in bits."""
        import numpy as np
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint32).reshape(-1, 3))
        out = np.zeros(len(r), dtype=np.float64)
        fn = self.ctx.lib.zmx_block_costs
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        self.ctx._check(fn(self.ctx.handle, self.handle, len(r), r.ctypes.data_as(ctypes.c_void_p),
                           out.ctypes.data_as(ctypes.c_void_p)), "zmx_block_costs")
        return out

    def positions(self, pairs):
        """pairs = [(sequence, index)] -> the bytes that symbols [0, index) of the sequence stand for (zmx_cost_positions)."""
        import numpy as np
        q = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2))
        out = np.zeros(len(q), dtype=np.uint64)
        fn = self.ctx.lib.zmx_cost_positions
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        self.ctx._check(fn(self.ctx.handle, self.handle, len(q), q.ctypes.data_as(ctypes.c_void_p),
                           out.ctypes.data_as(ctypes.c_void_p)), "zmx_cost_positions")
        return out

    def free(self):
        if self.handle:
            fn = self.ctx.lib.zmx_cost_stores_free
            fn.restype = None
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            fn(self.ctx.handle, self.handle)
            self.handle = None


class DeviceBits:
    """The bits of one Tables.encode_blocks_device call, in device memory (zmx_bits)."""

    def __init__(self, ctx, handle, njobs):
        self.ctx, self.handle, self.njobs = ctx, handle, njobs

    def job(self, j):
        """(device pointer, bit_start, nbits) of job j: its symbols are bits [bit_start, bit_start + nbits) of the string
        at the pointer; the bits in front of them are zero."""
        ptr, start, nbits = ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_uint64(0)
        fn = self.ctx.lib.zmx_bits_job
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                       ctypes.POINTER(ctypes.c_uint64)]
        self.ctx._check(fn(self.handle, j, ctypes.byref(ptr), ctypes.byref(start), ctypes.byref(nbits)), "zmx_bits_job")
        return int(ptr.value or 0), int(start.value), int(nbits.value)

    def free(self):
        if self.handle:
            fn = self.ctx.lib.zmx_bits_free
            fn.restype = None
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            fn(self.ctx.handle, self.handle)
            self.handle = ctypes.c_void_p()


class Tables:
    def __init__(self, ctx, handle, blocks):
        self.ctx, self.handle, self.blocks = ctx, handle, blocks

    def free(self):
        if self.handle:
            self.ctx.lib.zmx_tables_free(self.ctx.handle, self.handle)
            self.handle = None

    def trim(self):
        """zmx_tables_trim: everything but the two stores goes back to the pool."""
        self.ctx._check(self.ctx.lib.zmx_tables_trim(self.ctx.handle, self.handle), "zmx_tables_trim")

    def greedy(self, slot=0):
        import numpy as np
        nb = len(self.blocks)
        nsym = np.zeros(nb, dtype=np.uint32)
        hist = np.zeros((nb, ZMX_HIST), dtype=np.uint32)
        self.ctx._check(self.ctx.lib.zmx_lz77_greedy(self.ctx.handle, self.handle, slot,
                                                     nsym.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                     hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
                        "zmx_lz77_greedy")
        return nsym, hist

    def squeeze_run(self, cost, mincost, slot):
        import numpy as np
        nb = len(self.blocks)
        cost = np.ascontiguousarray(cost, dtype=np.float64)
        mincost = np.ascontiguousarray(mincost, dtype=np.float64)
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        nsym = np.zeros(nb, dtype=np.uint32)
        hist = np.zeros((nb, ZMX_HIST), dtype=np.uint32)
        self.ctx._check(self.ctx.lib.zmx_squeeze_run(self.ctx.handle, self.handle,
                                                     cost.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                     mincost.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                     slot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                     nsym.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                     hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
                        "zmx_squeeze_run")
        return nsym, hist

    def trace(self, length_arrays, slot):
        """zmx_trace_length_arrays: the trace kernels of a squeeze run on the given length arrays (one per block,
        blocksize + 1 cells each) -> (nsym, hist), the symbols in store slot[b] of block b."""
        import numpy as np
        nb = len(length_arrays)
        las = [np.ascontiguousarray(a, dtype=np.uint16) for a in length_arrays]
        ptrs = (ctypes.c_void_p * max(nb, 1))(*[a.ctypes.data for a in las])
        entries = (ctypes.c_size_t * max(nb, 1))(*[a.size for a in las])
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        if slot.size != nb:
            raise ValueError("Tables.trace: one slot per length array")
        nsym = np.zeros(max(nb, len(self.blocks)), dtype=np.uint32)
        hist = np.zeros((max(nb, len(self.blocks)), ZMX_HIST), dtype=np.uint32)
        # (bound here, not in bind(): an older build selected by ZOPFLI_AMD_LIB for an A/B still loads)
        fn = self.ctx.lib.zmx_trace_length_arrays
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self.ctx._check(fn(self.ctx.handle, self.handle, nb, ctypes.cast(ptrs, ctypes.c_void_p),
                           ctypes.cast(entries, ctypes.c_void_p), slot.ctypes.data_as(ctypes.c_void_p),
                           nsym.ctypes.data_as(ctypes.c_void_p), hist.ctypes.data_as(ctypes.c_void_p)),
                        "zmx_trace_length_arrays")
        return nsym[:nb], hist[:nb]

    def store(self, block, slot, nsym):
        import numpy as np
        ll = np.zeros(max(int(nsym), 1), dtype=np.uint16)
        dd = np.zeros(max(int(nsym), 1), dtype=np.uint16)
        self.ctx._check(self.ctx.lib.zmx_store_download(self.ctx.handle, self.handle, block, slot,
                                                        ll.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                                        dd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), int(nsym)),
                        "zmx_store_download")
        return ll[:int(nsym)], dd[:int(nsym)]

    def verify_stores(self, blocks, slots, nsyms):
        """zmx_verify_stores: raises RuntimeError naming the first symbol that does not stand for the input's bytes."""
        n = len(blocks)
        fn = self.ctx.lib.zmx_verify_stores
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        b = (ctypes.c_size_t * n)(*map(int, blocks))
        s = (ctypes.c_int32 * n)(*map(int, slots))
        k = (ctypes.c_size_t * n)(*map(int, nsyms))
        self.ctx._check(fn(self.ctx.handle, self.handle, n, ctypes.cast(b, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
                           ctypes.cast(k, ctypes.c_void_p)), "zmx_verify_stores")

    def encode_blocks(self, jobs, codes, slack=False):
        """zmx_encode_blocks: jobs = [(block, slot, nsym, bit_start, nbits)], codes = uint32 [njobs, 320]
        (reversed code | length << 16).  Returns one bytes object per job (header bits zero); slack=True: with the 8
        bytes allocated behind each output, which the library must leave alone."""
        import numpy as np

        class Job(ctypes.Structure):
            _fields_ = [("block", ctypes.c_uint32), ("slot", ctypes.c_int32), ("nsym", ctypes.c_uint32),
                        ("bit_start", ctypes.c_uint32), ("nbits", ctypes.c_uint64)]
        n = len(jobs)
        arr = (Job * n)(*[Job(*map(int, j)) for j in jobs])
        codes = np.ascontiguousarray(codes, dtype=np.uint32).reshape(n, 320)
        bufs = [np.zeros((int(j[3]) + int(j[4]) + 7) // 8 + 8, dtype=np.uint8) for j in jobs]
        ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
        fn = self.ctx.lib.zmx_encode_blocks
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self.ctx._check(fn(self.ctx.handle, self.handle, n, ctypes.cast(arr, ctypes.c_void_p),
                           codes.ctypes.data_as(ctypes.c_void_p), ctypes.cast(ptrs, ctypes.c_void_p)), "zmx_encode_blocks")
        if slack:
            return [bytes(b) for b in bufs]
        return [bytes(b[:(int(j[3]) + int(j[4]) + 7) // 8]) for b, j in zip(bufs, jobs)]

    def encode_blocks_device(self, jobs, codes):
        """zmx_encode_blocks_device: encode_blocks whose bits stay in device memory.  Returns a DeviceBits: job j's bit
        string is at the device pointer ptr(j), its symbols from bit bit_start(j) on, nbits(j) of them; free() it on
        this context when nothing reads it any more."""
        import numpy as np

        class Job(ctypes.Structure):
            _fields_ = [("block", ctypes.c_uint32), ("slot", ctypes.c_int32), ("nsym", ctypes.c_uint32),
                        ("bit_start", ctypes.c_uint32), ("nbits", ctypes.c_uint64)]
        n = len(jobs)
        arr = (Job * max(n, 1))(*[Job(*map(int, j)) for j in jobs])
        codes = np.ascontiguousarray(codes, dtype=np.uint32).reshape(n, 320)
        handle = ctypes.c_void_p()
        fn = self.ctx.lib.zmx_encode_blocks_device
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.POINTER(ctypes.c_void_p)]
        self.ctx._check(fn(self.ctx.handle, self.handle, n, ctypes.cast(arr, ctypes.c_void_p),
                           codes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(handle)), "zmx_encode_blocks_device")
        return DeviceBits(self.ctx, handle, n)

    def find_longest_match(self, block, pos):
        import numpy as np
        sub = np.zeros(259, dtype=np.uint16)
        d, l = ctypes.c_uint16(0), ctypes.c_uint16(0)
        self.ctx._check(self.ctx.lib.zmx_find_longest_match(self.ctx.handle, self.handle, block, pos,
                                                            sub.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                                            ctypes.byref(d), ctypes.byref(l)),
                        "zmx_find_longest_match")
        return l.value, d.value, sub

    def match_digest(self):
        """zmx_match_digest: a digest of every match record of these tables."""
        out = (ctypes.c_uint64 * 2)()
        fn = self.ctx.lib.zmx_match_digest
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        self.ctx._check(fn(self.ctx.handle, self.handle, out), "zmx_match_digest")
        return (int(out[0]), int(out[1]))

    def hash_links(self, block):
        """same[], prev1[], prev2[] of the block's positions from windowstart on (zmx_hash_links_download)."""
        import numpy as np
        s, e = self.blocks[block]
        n = e - self.ctx.window_start(s)
        arrs = [np.zeros(max(n, 1), dtype=np.uint16) for _ in range(3)]
        ptrs = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)) for a in arrs]
        self.ctx._check(self.ctx.lib.zmx_hash_links_download(self.ctx.handle, self.handle, block, *ptrs),
                        "zmx_hash_links_download")
        return [a[:n] for a in arrs]

    def length_array(self, block):
        import numpy as np
        s, e = self.blocks[block]
        la = np.zeros(e - s + 1, dtype=np.uint16)
        self.ctx._check(self.ctx.lib.zmx_length_array_download(self.ctx.handle, self.handle, block,
                                                               la.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))),
                        "zmx_length_array_download")
        return la

    def dp_rows(self, block):
        """zmx_dp_rows_download: the DP row layout of one block as a dict of numpy arrays — "roff" and "flags" (dph's
        two words per position), "kend", "shortcut", "run_row", "literal", "codeless" (the fields of "flags"),
        "block_edges" (int), "codes" (uint16[block_edges]), "winflag", "winroff" (uint32[W]) and "wmeta"
        (uint32[W, 40]), W = (B + 31) // 32 + 1."""
        import numpy as np
        fn = self.ctx.lib.zmx_dp_rows_download
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)] + [ctypes.c_void_p] * 5
        edges = ctypes.c_uint64(0)
        # (the sizes first; a block or tables that the entry refuses are refused here)
        self.ctx._check(fn(self.ctx.handle, self.handle, block, ctypes.byref(edges), None, None, None, None, None),
                        "zmx_dp_rows_download")
        s, e = self.blocks[block]
        B = e - s
        W = (B + 31) // 32 + 1
        dph = np.zeros((max(B, 1), 2), dtype=np.uint32)
        codes = np.zeros(max(edges.value, 1), dtype=np.uint16)
        winflag = np.zeros(W, dtype=np.uint32)
        winroff = np.zeros(W, dtype=np.uint32)
        wmeta = np.zeros((W, 40), dtype=np.uint32)
        self.ctx._check(fn(self.ctx.handle, self.handle, block, ctypes.byref(edges), dph.ctypes.data, codes.ctypes.data,
                           winflag.ctypes.data, winroff.ctypes.data, wmeta.ctypes.data), "zmx_dp_rows_download")
        flags = dph[:B, 1].copy()
        return {"roff": dph[:B, 0].copy(), "flags": flags, "kend": flags & 0xffff, "shortcut": (flags >> 16) & 1,
                "run_row": (flags >> 17) & 1, "literal": (flags >> 18) & 0xff, "codeless": (flags >> 26) & 1,
                "block_edges": int(edges.value), "codes": codes[:edges.value], "winflag": winflag, "winroff": winroff,
                "wmeta": wmeta}

    def chain_tasks(self):
        """zmx_chain_tasks_download: the chain's task set-up of the whole table set as a dict — "tasks" (uint32
        [ntasks, 4]: block, q, pout, pend, after the merge), "task_off" (uint32[nb + 1]), "merged" (int), "wg_tasks"
        (uint32[ntasks]: the text list, then the run list), "wg_desc" (uint32[n_wg + n_wg_runs, 2]: first entry,
        entries), "n_wg", "n_wg_runs" (int) and "kind" (uint32[ntasks]: 1 for the tasks of the run list)."""
        import numpy as np
        fn = self.ctx.lib.zmx_chain_tasks_download
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)] + [ctypes.c_void_p] * 4
        counts = (ctypes.c_uint64 * 4)()
        # (the sizes first; tables that the entry refuses are refused here)
        self.ctx._check(fn(self.ctx.handle, self.handle, counts, None, None, None, None), "zmx_chain_tasks_download")
        nt, merged, n_wg, n_wg_runs = (int(v) for v in counts)
        tasks = np.zeros((max(nt, 1), 4), dtype=np.uint32)
        task_off = np.zeros(len(self.blocks) + 1, dtype=np.uint32)
        wg_tasks = np.zeros(max(nt, 1), dtype=np.uint32)
        wg_desc = np.zeros((max(n_wg + n_wg_runs, 1), 2), dtype=np.uint32)
        self.ctx._check(fn(self.ctx.handle, self.handle, counts, tasks.ctypes.data, task_off.ctypes.data, wg_tasks.ctypes.data,
                           wg_desc.ctypes.data), "zmx_chain_tasks_download")
        wg_desc = wg_desc[:n_wg + n_wg_runs]
        kind = np.zeros(nt, dtype=np.uint32)
        for first, n in wg_desc[n_wg:]:
            kind[wg_tasks[int(first):int(first) + int(n)]] = 1
        return {"tasks": tasks[:nt], "task_off": task_off, "merged": merged, "wg_tasks": wg_tasks[:nt], "wg_desc": wg_desc,
                "n_wg": n_wg, "n_wg_runs": n_wg_runs, "kind": kind}
