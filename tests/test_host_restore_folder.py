"""CPU-only: the host side of DiffusiveRestoration.restore_folder (photographs at their own size, without ground truth) -- padded sizes, the
per-file seed, the folder listing with its naming rule, the memory estimate."""
import os
import zlib

import numpy as np
import pytest

from wavedm_amd import datasets, imageio, restoration
from wavedm_amd import procedural as P


@pytest.mark.parametrize("args, want", [((1, 1, 16, 64), (64, 64)), ((70, 93, 16, 64), (80, 96)), ((64, 64, 16, 64), (64, 64)),
                                        ((480, 720, 16, 256), (480, 720)), ((65, 300, 16, 64), (80, 304))])
def test_padded_size(args, want):
    assert imageio.padded_size(*args) == want


def test_padded_size_defaults_and_refusals():
    assert imageio.padded_size(70, 93) == (80, 96) and imageio.padded_size(3, 5, 4) == (4, 8)
    with pytest.raises(ValueError):
        imageio.padded_size(0, 5)
    with pytest.raises(ValueError):
        imageio.padded_size(5, 5, 16, 40)                     # min_side is itself a multiple of `multiple`


def test_file_seed_is_the_documented_formula():
    assert restoration.file_seed(61, "a.png") == ((61 & 0x7FFFFFFF) << 32) | zlib.crc32("a.png".encode("utf-8"))
    assert restoration.file_seed(0, "sub/b.jpg") == zlib.crc32("sub/b.jpg".encode("utf-8"))
    assert restoration.file_seed(61, "a.png") != restoration.file_seed(61, "b.png") != restoration.file_seed(62, "b.png")
    assert 0 <= restoration.file_seed(-1, "ä/ü.png") < 1 << 63                          # any int seed, any name: a seed torch's generators take


def _touch_image(path, size=(5, 4)):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.zeros((size[1], size[0], 3), np.uint8)).save(path)


@pytest.fixture()
def folder(tmp_path):
    root = tmp_path / "in"
    for name in ("b.png", "a.JPG", "c.jpeg", "Z.bmp", "d.TIFF", "e.tif", "sub/x.png", "sub/deep/y.PNG"):
        _touch_image(str(root / name))
    for name in ("notes.txt", "thumbs.db", "f.png.bak", "sub/readme.md", "g.gif"):
        os.makedirs(os.path.dirname(str(root / name)), exist_ok=True)
        (root / name).write_bytes(b"not an image")
    return root


def test_image_folder_listing(folder):
    flat = datasets.ImageFolder(str(folder))
    assert flat.names == ["Z.bmp", "a.JPG", "b.png", "c.jpeg", "d.TIFF", "e.tif"] and len(flat) == 6          # sorted by name; other extensions ignored
    rec = datasets.ImageFolder(str(folder), recursive=True)
    assert rec.names == ["Z.bmp", "a.JPG", "b.png", "c.jpeg", "d.TIFF", "e.tif", "sub/deep/y.PNG", "sub/x.png"]
    assert datasets.ImageFolder(str(folder), recursive=True, shard=(1, 3)).names == rec.names[1::3] == ["a.JPG", "d.TIFF", "sub/x.png"]
    with pytest.raises(ValueError):
        datasets.ImageFolder(str(folder), shard=(3, 3))
    img, name = rec[6]
    assert name == "sub/deep/y.PNG" and img.dtype.is_floating_point is False and tuple(img.shape) == (4, 5, 3)
    assert [n for _, n in rec] == rec.names
    assert set(datasets.IMAGE_EXTENSIONS) == {".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp"}


def test_output_names_and_collisions(folder):
    rec = datasets.ImageFolder(str(folder), recursive=True)
    assert datasets.output_names(rec.names) == ["Z.png", "a.png", "b.png", "c.png", "d.png", "e.png", "sub/deep/y.png", "sub/x.png"]
    _touch_image(str(folder / "a.png"))
    with pytest.raises(ValueError, match=r"a\.JPG.*a\.png"):
        datasets.output_names(datasets.ImageFolder(str(folder)).names)


def test_undecodable_file_is_an_oserror_naming_it(folder):
    (folder / "broken.png").write_bytes(b"\x89PNG\r\n\x1a\n garbage")
    ds = datasets.ImageFolder(str(folder))
    with pytest.raises(OSError, match="broken.png"):
        ds[ds.names.index("broken.png")]


def test_image_loader_yields_single_items(folder):
    loader = datasets.image_loader(str(folder), 0, P.reduced_config(), recursive=True)
    items = list(loader)
    assert [n for _, n in items] == datasets.ImageFolder(str(folder), recursive=True).names
    assert all(tuple(x.shape) == (4, 5, 3) and x.dtype.is_floating_point is False for x, _ in items)


def test_estimate_restore_bytes_terms_and_monotonicity():
    cfg = P.reduced_config()                                  # 16-pixel wavelet-domain patches of 96 channels, pred_channels 3
    p, cin, pc = 16, P.unet_in_channels(cfg), 3
    for (h, w, n_img, dtype, elsize) in ((70, 93, 1, "f32", 4), (70, 93, 3, "bf16", 2), (100, 130, 2, "f16", 2), (33, 40, 1, "f32x3", 4)):
        hp, wp = imageio.padded_size(h, w, 16, 4 * p)
        n = n_img * len(range(0, hp // 4 - p + 1, 4)) * len(range(0, wp // 4 - p + 1, 4))              # r = 4 divides every padded size here
        t = restoration.restore_terms(h, w, n_img, cfg, 32, dtype, r=4, steps=6)
        assert t["x96"] == n * p * p * cin * elsize and t["eps"] == n * pc * p * p * 4
        assert t["hfrm"] > 0 and t["unet"] > 0 and t["full"] >= n_img * 4 * 3 * hp * wp
        assert restoration.estimate_restore_bytes(h, w, n_img, cfg, 32, dtype, r=4, steps=6) == sum(t.values())
    est = lambda h, w, n: restoration.estimate_restore_bytes(h, w, n, cfg, 32, "f32", r=4, steps=6)
    hs = [1, 17, 64, 65, 70, 80, 81, 130, 300]
    for a, b in zip(hs, hs[1:]):
        assert est(a, 93, 2) <= est(b, 93, 2) and est(70, a, 2) <= est(70, b, 2)
    assert all(est(70, 93, n) <= est(70, 93, n + 1) for n in range(1, 9))
    assert est(70, 93, 1) < est(70, 93, 2) < est(300, 300, 2)
    # every band diffused: no HFRM term
    assert restoration.restore_terms(70, 93, 1, P.pred_channels_config(48), 32, "f32", r=4, steps=6)["hfrm"] == 0
