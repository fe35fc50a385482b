"""ZMX_PNG_FILTER_AUTO and zmx_png_choose_strategy_device: zopflipng's own choice of the filter strategy for an image in
device memory.  The images are tests/png_trial_cases.py's: the ten shapes of png_encode_cases; "all-zero" (trials 0, m and
e tie: zero wins), "vgrad-w1" (a column of pixels: Up and Paeth filter alike, two wins), "smooth-rows" (one, tied with
entropy), "smooth-columns" (two), "plane" (four), "halves-noisy" (minimum sum), "halves" (entropy; with suited predefined
types those win, with poor ones they lose; on "plane" they tie with four and lose), "icon-12" (40 x 40, 12 colours: the
palette file is below 4096 bytes and the RGB second try decides inside every trial), "hidden-rows" (--lossy_transparent
changes the choice from entropy to minimum sum).  The eight trial sizes and the choice are zopflipng's own
(tests/golden/png_trials.json); the AUTO entries must give the file the same entry gives with the chosen strategy, and
the file oracle/_ref/zopflipng_ref writes without --filters where that was built.  numiterations 2 throughout."""
import os
import subprocess

import numpy as np
import pytest
import torch

import png_encode_cases as ec
import png_trial_cases as tc
from png_rows_cases import filter_rows
from zopfli_amd import Context, ZopfliOptions, api
from zopfli_amd._build import PNG_REF

pytestmark = pytest.mark.gpu

ITERATIONS = 2
ORDER = [0, 1, 2, 3, 4, 5, 6, 8]      # trial k's ZMX_PNG_FILTER_*: 0 .. 4, MINSUM, ENTROPY, PREDEFINED


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    return tc.golden()["images"]


def _on_device(name):
    d = torch.from_numpy(tc.image(name).copy()).cuda()
    torch.cuda.synchronize()
    return d


def _image(name, d_img):
    nm, w, h, ct, depth = tc.image_case(name)
    return (d_img.data_ptr(), w, h, ct, depth)


def _entry(keep):
    return api.png_encode_device if keep else api.png_optimize_device


def _reference(tmp_path, name, keep, lossy, types):
    """The all-reference zopflipng's file without --filters, or None where it was not built."""
    if not os.path.exists(PNG_REF):
        return None
    nm, w, h, ct, depth = tc.image_case(name)
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    carried = np.zeros(h, dtype=np.uint8) if types is None else types
    with open(src, "wb") as f:
        f.write(ec.plain_png((w, h, ct, depth), filter_rows(tc.image(name), ec.CHANNELS[ct] * depth // 8, carried)))
    flags = ["-y", "--always_zopflify", f"--iterations={ITERATIONS}"] + (["--keepcolortype"] if keep else []) + \
        (["--lossy_transparent"] if lossy else [])
    r = subprocess.run([PNG_REF] + flags + [src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", tc.IMAGE_IDS)
def test_choice_and_file(ctx, gpu_lib, gold, tmp_path, name):
    d_img = _on_device(name)
    image = _image(name, d_img)
    opts = ZopfliOptions(ITERATIONS)
    for keep in (1, 0):
        g = gold[f"{name}|{keep}|0|-"]
        strategy, sizes = ctx.png_choose_strategy_device(image, reduce_color=not keep)
        assert sizes[:7] == g["sizes"][:7] and sizes[7] == 0, (name, keep, sizes, g["sizes"])
        assert strategy == ORDER[g["best"]], (name, keep)
        png = _entry(keep)(image, api.PNG_FILTER_AUTO, opts, lib=gpu_lib)
        assert api.last_input_traffic(gpu_lib)[0] == 0, "pixels went host to device"
        assert png == _entry(keep)(image, strategy, opts, lib=gpu_lib), (name, keep)
        assert png == _entry(keep)(image, "auto", opts, lib=gpu_lib)
        ref = _reference(tmp_path, name, keep, 0, None)
        assert ref is None or png == ref, (name, keep, "zopflipng_ref")
    assert np.array_equal(d_img.cpu().numpy(), tc.image(name)), "the image changed"


@pytest.mark.parametrize("label", list(tc.PREDEFINED_RUNS))
def test_predefined_trial(ctx, gpu_lib, gold, tmp_path, label):
    name, make = tc.PREDEFINED_RUNS[label]
    types = make(tc.image_case(name)[2])
    d_img = _on_device(name)
    image = _image(name, d_img)
    opts = ZopfliOptions(ITERATIONS)
    for keep in (1, 0):
        g = gold[f"{name}|{keep}|0|{label}"]
        strategy, sizes = ctx.png_choose_strategy_device(image, reduce_color=not keep, predefined=types)
        assert sizes == g["sizes"] and strategy == ORDER[g["best"]], (label, keep, sizes, g)
        png = _entry(keep)(image, api.PNG_FILTER_AUTO, opts, predefined=types, lib=gpu_lib)
        assert png == _entry(keep)(image, strategy, opts, predefined=types, lib=gpu_lib), (label, keep)
        ref = _reference(tmp_path, name, keep, 0, types)
        assert ref is None or png == ref, (label, keep, "zopflipng_ref")
    with pytest.raises(RuntimeError, match="predefined type 5"):
        ctx.png_choose_strategy_device(image, predefined=[5] * len(types))


def test_lossy_comes_before_the_choice(ctx, gpu_lib, gold, tmp_path):
    name = "hidden-rows"
    d_img = _on_device(name)
    image = _image(name, d_img)
    opts = ZopfliOptions(ITERATIONS)
    for keep in (1, 0):
        plain, lossy = gold[f"{name}|{keep}|0|-"]["best"], gold[f"{name}|{keep}|1|-"]["best"]
        assert plain != lossy
        png = _entry(keep)(image, api.PNG_FILTER_AUTO, opts, lib=gpu_lib, lossy_transparent=True)
        assert api.last_input_traffic(gpu_lib)[0] == 0
        assert png == _entry(keep)(image, ORDER[lossy], opts, lib=gpu_lib, lossy_transparent=True), keep
        if keep:   # (reduced, minimum sum and entropy tie on the rewritten image and pick the same types: one file)
            assert png != _entry(keep)(image, ORDER[plain], opts, lib=gpu_lib, lossy_transparent=True), keep
        ref = _reference(tmp_path, name, keep, 1, None)
        assert ref is None or png == ref, (keep, "zopflipng_ref")
    assert np.array_equal(d_img.cpu().numpy(), tc.image(name)), "the image changed"


def test_batches_equal_singles(gpu_lib):
    names = ["shape-" + ec.shape_id(s) for s in ec.SHAPES] + ["all-zero", "vgrad-w1", "smooth-rows", "halves", "halves-noisy", "icon-12",
                                                                 "hidden-rows"]
    imgs = [_on_device(n) for n in names]
    images = [_image(n, d) for n, d in zip(names, imgs)]
    opts = ZopfliOptions(ITERATIONS)
    for single, batch in ((api.png_encode_device, api.png_encode_device_batch), (api.png_optimize_device, api.png_optimize_device_batch)):
        for lossy in (False, True):
            singles = [single(im, api.PNG_FILTER_AUTO, opts, lib=gpu_lib, lossy_transparent=lossy) for im in images]
            assert batch(images, api.PNG_FILTER_AUTO, opts, lib=gpu_lib, lossy_transparent=lossy) == singles
            assert api.last_input_traffic(gpu_lib)[0] == 0
            order = [(5 * i + 2) % len(images) for i in range(len(images))]
            assert sorted(order) == list(range(len(images)))
            assert batch([images[i] for i in order], api.PNG_FILTER_AUTO, opts, lib=gpu_lib, lossy_transparent=lossy) == [singles[i] for i in order]
    for n, d in zip(names, imgs):
        assert np.array_equal(d.cpu().numpy(), tc.image(n)), "an image changed"


def test_refusals(ctx, gpu_lib):
    d = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = d.data_ptr()
    for what, image in (("width 0", (p, 0, 16, 6, 8)), ("palette input", (p, 16, 16, 3, 8)), ("null pixels", (0, 16, 16, 6, 8)),
                        ("pixels leave their allocation", (p, 4096, 4096, 6, 8))):
        with pytest.raises(RuntimeError, match="zmx_png_choose_strategy_device"):
            ctx.png_choose_strategy_device(image)
    # the batches still refuse predefined types, and strategy 9 is still none
    with pytest.raises(RuntimeError):
        api.png_encode_device_batch([(p, 16, 16, 6, 8)], 8, ZopfliOptions(ITERATIONS), lib=gpu_lib)
    with pytest.raises(RuntimeError):
        api.png_encode_device((p, 16, 16, 6, 8), 9, ZopfliOptions(ITERATIONS), lib=gpu_lib)
    strategy, sizes = ctx.png_choose_strategy_device((p, 16, 16, 6, 8))
    assert strategy == 0 and sizes[7] == 0 and min(sizes[:7]) == sizes[0]
