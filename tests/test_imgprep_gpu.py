"""K0 (csrc/imgprep.hip) on the GPU is byte-identical to the reference's preprocessing:
PIL bicubic shortest-edge resize + centre crop (app/encoders/preprocess.py:to_u8_224, the
restatement of CLIPImageProcessor pinned in test_compat_cpu.py), on one mixed-size batch:
downscale, upscale, unchanged width or height, identity, extreme aspect ratios, a 12 MP
photo size."""
from __future__ import annotations

import numpy as np
import pytest
from PIL import Image

from app.encoders.preprocess import to_u8_224

pytestmark = pytest.mark.gpu

SIZES = [(640, 480), (480, 640), (224, 224), (225, 224), (224, 225), (224, 900), (100, 150), (1000, 223),
         (223, 1000), (333, 777), (1920, 1080), (50, 60), (17, 400), (4000, 3000)]


def _img(w, h, seed):
    rng = np.random.default_rng(seed)
    if seed % 2:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 127 // max(w + h, 1))], -1)
    return np.clip(base + rng.integers(-8, 9, base.shape), 0, 255).astype(np.uint8)


def test_resize_crop_device_bit_exact(cuda):
    from app.encoders.preprocess import resize_crop_device

    imgs = [_img(w, h, i) for i, (w, h) in enumerate(SIZES)]
    got = resize_crop_device(imgs).cpu().numpy()
    for i, a in enumerate(imgs):
        np.testing.assert_array_equal(got[i], to_u8_224(Image.fromarray(a)), err_msg=str(SIZES[i]))


def test_load_batch_device_files(cuda, tmp_path):
    """Decode (host) + resize/crop (GPU) from files, incl. grayscale and RGBA sources."""
    from app.encoders.preprocess import load_batch, load_batch_device

    paths = []
    for i, (w, h, mode) in enumerate([(300, 200, "RGB"), (200, 300, "L"), (512, 512, "RGBA"), (224, 224, "RGB")]):
        a = _img(w, h, 100 + i)
        im = Image.fromarray(a).convert(mode)
        p = tmp_path / f"im{i}.png"
        im.save(p)
        paths.append(p)
    np.testing.assert_array_equal(load_batch_device(paths).cpu().numpy(), load_batch(paths))
    assert load_batch_device([]).shape == (0, 224, 224, 3)


# ---- the kernel's own switches and edges, every image against to_u8_224(Image.fromarray(a), size) ----

RH_LDS = 6144  # csrc/imgprep.hip: ints of LDS for one image's column tap table


def _resized(w, h, size):
    """(new width, new height) of the shortest-edge resize, as to_u8_224 computes them."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (size, new_long) if w <= h else (new_long, size)


def _taps(in_size, out_size):
    """Taps per output position of Pillow's bicubic pass (Resample.c precompute_coeffs): one identity
    tap when the size does not change, else ceil(2 * max(scale, 1)) * 2 + 1."""
    if in_size == out_size:
        return 1
    scale = float(np.float32(in_size)) / out_size
    return int(np.ceil(2.0 * max(scale, 1.0))) * 2 + 1


def _column_table_in_lds(w, h, size):
    """The kernel's condition for staging the column taps in LDS: size rows of [xmin, n, taps...]."""
    return size * (2 + _taps(w, _resized(w, h, size)[0])) <= RH_LDS


def _check_batch(imgs, size=224):
    from app.encoders.preprocess import resize_crop_device

    got = resize_crop_device(imgs, size=size).cpu().numpy()
    assert got.shape == (len(imgs), size, size, 3)
    refs = []
    for i, a in enumerate(imgs):
        ref = to_u8_224(Image.fromarray(a), size)
        np.testing.assert_array_equal(got[i], ref, err_msg=f"image {i}: {a.shape[1]}x{a.shape[0]} -> {size}")
        refs.append(ref)
    return refs


def test_tap_table_boundary_224(cuda):
    """Scales 5.996 and 6 (25 taps, 224 * 27 ints: LDS) against 6.004 (27 taps, 224 * 29: global)."""
    sizes = [(1343, 1343), (1344, 1344), (1345, 1345), (1345, 1400)]
    assert [_taps(w, 224) for w, _ in sizes] == [25, 25, 27, 27]
    assert [_column_table_in_lds(w, h, 224) for w, h in sizes] == [True, True, False, False]
    assert 224 * (2 + 25) <= RH_LDS < 224 * (2 + 27)
    _check_batch([_img(w, h, 31 + 2 * i) for i, (w, h) in enumerate(sizes)])


@pytest.mark.parametrize("size", [32, 336])
def test_other_output_sizes(cuda, size):
    """A downscale, an upscale, an unchanged width, an unchanged height and the identity at another
    output size; at 336 also the two source widths on either side of its LDS / global switch."""
    big, small = 2 * size + 60, size // 2 + 5
    sizes = [(big + 35, big), (small, small + 11), (size, size + 50), (size + 50, size), (size, size)]
    if size == 336:
        first_global = next(w for w in range(size, 20 * size) if not _column_table_in_lds(w, w, size))
        assert _column_table_in_lds(first_global - 1, first_global - 1, size) and first_global * first_global * 3 < 6e6
        assert _taps(first_global, size) == _taps(first_global - 1, size) + 2
        sizes += [(first_global - 1, first_global - 1), (first_global, first_global)]
    else:
        assert all(_column_table_in_lds(w, h, size) for w, h in sizes)
    _check_batch([_img(w, h, 51 + 2 * i) for i, (w, h) in enumerate(sizes)], size)


def test_tiny_and_thin_sources(cuda):
    sizes = [(1, 1), (1, 2), (2, 1), (2, 3), (1, 50), (50, 1), (3, 2000), (2000, 3)]
    _check_batch([_img(w, h, 71 + 2 * i) for i, (w, h) in enumerate(sizes)])


def _pattern(kind, w, h, framed=False):
    """0 / 255 patterns of one-pixel (or 2 x 2) period; ``framed`` lays solid black and white 32-pixel
    blocks among cells of the pattern, so that a downscale still meets full-contrast edges."""
    y, x = np.mgrid[0:h, 0:w]
    m = {"checker1": (x + y) % 2, "vstripes": x % 2, "hstripes": y % 2, "checker2": (x // 2 + y // 2) % 2}[kind]
    if framed:
        cell = (x // 32 + 2 * (y // 32)) % 3
        m = np.where(cell == 0, m, cell - 1)
    return np.ascontiguousarray(np.repeat((m * 255).astype(np.uint8)[:, :, None], 3, axis=2))


def test_clamp_content(cuda):
    """Bicubic overshoot into both clamps of clip8. Upscaled (100 x 150) every pattern's reference
    output holds 0, 255 and grey in between. Downscaled (640 x 480, scale 2.14) a bare one- or
    two-pixel pattern averages out (the reference stays within 76..179), so it is compared as it is
    and the clamps are reached there by the framed variant of each pattern."""
    kinds = ("checker1", "vstripes", "hstripes", "checker2")
    imgs = [_pattern(k, 100, 150) for k in kinds] + [_pattern(k, 640, 480, framed=True) for k in kinds]
    bare = [_pattern(k, 640, 480) for k in kinds]
    refs = _check_batch(imgs + bare)
    for i, ref in enumerate(refs):
        grey = np.any((ref[8:-8, 8:-8] > 40) & (ref[8:-8, 8:-8] < 215))
        assert grey, f"image {i}: no grey interior pixel, the filter did not run"
        if i < len(imgs):
            assert (ref == 0).any() and (ref == 255).any(), f"image {i}: a clamp is not reached"
        else:  # the bare downscaled patterns: the claim of the docstring, held
            assert 76 <= ref.min() and ref.max() <= 179, f"image {i}: {ref.min()}..{ref.max()}"


def test_shared_tap_tables(cuda):
    """One size three times with different content, two sizes sharing only the column table, two
    sharing only the row table, and an unrelated size in between."""
    sizes = [(300, 200), (200, 300), (300, 200), (333, 777), (400, 200), (200, 400), (300, 200)]
    imgs = [_img(w, h, 90 + i) for i, (w, h) in enumerate(sizes)]
    assert not np.array_equal(imgs[0], imgs[2]) and not np.array_equal(imgs[2], imgs[6])
    _check_batch(imgs)


def test_single_image_and_unaligned_offsets(cuda):
    _check_batch([_img(101, 77, 3)])
    sizes = [(101, 77), (33, 51), (75, 35), (129, 131), (224, 224)]
    imgs = [_img(w, h, 110 + i) for i, (w, h) in enumerate(sizes)]
    assert all(a.size % 4 for a in imgs[:4])
    _check_batch(imgs)
