"""Build recipes for the native pieces (gfx950 only, in-tree outputs)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zopfli_amd", "csrc")
LIB = os.path.join(ROOT, "zopfli_amd", "libzopfli_amd.so")
# the reference's shared library is libzopfli.so.1 (Makefile:45): the same file under that name, so that
# a program linked against the reference's library picks this one up from LD_LIBRARY_PATH
LIB_SONAME = os.path.join(ROOT, "zopfli_amd", "libzopfli.so.1")
DATAGEN = os.path.join(CSRC, "tools", "libzopfli_datagen.so")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _sources():
    host = os.path.join(CSRC, "host")
    dev = os.path.join(CSRC, "device")
    cc = sorted(os.path.join(host, f) for f in os.listdir(host) if f.endswith(".cc"))
    hdr = [os.path.join(d, f) for d in (host, dev) for f in os.listdir(d) if f.endswith(".h")]
    hdr.append(os.path.join(ROOT, "include", "zopfli_amd.h"))
    hdr.append(os.path.join(CSRC, "libzopfli_amd.map"))
    return os.path.join(dev, "zmx_hip.hip"), cc, hdr


def build_product(force=False):
    """hipcc --offload-arch=gfx950: HIP device layer + C++ host code -> libzopfli_amd.so."""
    hip, cc, hdr = _sources()
    if not force and not _newer(LIB, [hip] + cc + hdr) and os.path.exists(LIB_SONAME):
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
           "-fvisibility=hidden", "-Wl,-soname,libzopfli.so.1",
           "-Wl,--version-script=" + os.path.join(CSRC, "libzopfli_amd.map"),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "host"),
           "-I" + os.path.join(CSRC, "device"), hip] + cc + ["-o", LIB, "-lpthread", "-ldl"]
    subprocess.check_call(cmd)
    shutil.copyfile(LIB, LIB_SONAME)   # (a copy, not a symlink: it has to survive the snapshot to the GPU box)
    return LIB


def build_datagen(force=False):
    src = os.path.join(CSRC, "tools", "datagen.c")
    if force or _newer(DATAGEN, [src]):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", DATAGEN, src])
    return DATAGEN


def build_oracle():
    """Test infrastructure: the C restatement and, where the reference's tree is at hand, everything compiled from it
    (oracle/Makefile: the real reference, its CLI and zopflipng with and without libzopfli_amd.so, libzopflipng_amd.so,
    LodePNG's filter) into oracle/_ref/.  Without that tree the prebuilt oracle/_ref/ is kept as it is."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all"])


def build_hosttest():
    """Test infrastructure: product host sources + oracle-backed zmx layer (CPU-only checks)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib")])


# what oracle/Makefile compiles from the reference's tree (see there); binaries that use libzopfli_amd.so find it
# by an rpath relative to themselves, so oracle/_ref/ works wherever the tree is copied to
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
# the reference's own CLI (zopfli_bin.c) linked against libzopfli_amd.so: the drop-in claim of INTEGRATION.md section 1
REF_CLI = os.path.join(REF_DIR, "zopfli_ref_cli_amd")
# the reference as its own shared library (soname libzopfli.so.1) and its CLI linked against it with no rpath:
# LD_LIBRARY_PATH decides at run time whose libzopfli.so.1 it gets
REF_SO_DIR = os.path.join(REF_DIR, "reflib")
REF_CLI_DYN = os.path.join(REF_DIR, "zopfli_ref_cli_dyn")
# the reference's zopflipng on libzopfli_amd.so and all-reference
PNG_AMD = os.path.join(REF_DIR, "zopflipng_amd")
PNG_REF = os.path.join(REF_DIR, "zopflipng_ref")
# libzopflipng_amd.so: csrc/png/zopflipng_amd.cc with the ABI of the reference's zopflipng_lib.h on top of
# libzopfli_amd.so, LodePNG compiled in from LODEPNG_DIR (default: where the reference vendors it)
PNG_LIB = os.path.join(REF_DIR, "libzopflipng_amd.so")
# the reference's zopflipng command line on libzopflipng_amd.so, and LodePNG's own scanline filter behind a C symbol
PNG_AMD2 = os.path.join(REF_DIR, "zopflipng_amd2")
PNG_FILTER_REF = os.path.join(REF_DIR, "libpng_filter_ref.so")
# LodePNG's own LZ77 stage per deflate block and its zlib size behind C symbols (tests/hostlib/png_lodeflate_ref.cc)
PNG_LODEFLATE_REF = os.path.join(REF_DIR, "libpng_lodeflate_ref.so")
# LodePNG's fixed-tree deflate of every row under every filter type behind C symbols (tests/hostlib/png_brute_ref.cc)
PNG_BRUTE_REF = os.path.join(REF_DIR, "libpng_brute_ref.so")
