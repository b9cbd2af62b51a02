"""CPU-only: the host side of the mixed-size mode of restore_folder (args.mix_sizes) -- the ragged layout's tables and refusals, the grouping rule, the
memory estimate of a mixed call."""
import pytest

from wavedm_amd import restoration, sampling
from wavedm_amd import procedural as P

FIVE = [(16, 16), (16, 20), (28, 16), (20, 36), (16, 16)]         # the size lists of tests/test_gpu_ragged.py
SMALL = [(8, 12), (8, 8), (12, 20)]                               # p = 8: an image smaller than one workgroup, one that ends inside a 256-pixel block
THREE = [(16, 16), (20, 28), (24, 16)]


@pytest.mark.parametrize("sizes, p, r", [(FIVE, 16, 16), (SMALL, 8, 8), (THREE, 16, 4), ([(120, 180)], 64, 16)])
def test_layout_offsets_spans_and_alignment(sizes, p, r):
    lay = sampling.RaggedLayout(sizes, p, r)
    n = len(sizes)
    assert lay.nimg == n and lay.sizes == tuple(sizes) and lay.p == p
    # pixel offsets: the prefix sum of h * w; every block 16-byte aligned for every channel count
    assert lay.pix_off[0] == 0 and all(lay.pix_off[i + 1] - lay.pix_off[i] == h * w for i, (h, w) in enumerate(sizes))
    assert all((4 * C * o) % 16 == 0 for o in lay.pix_off for C in (1, 3, 5, 12, 45, 48))
    assert lay.numel(3) == 3 * sum(h * w for h, w in sizes) and lay.numel(48) == 16 * lay.numel(3)
    # 256-pixel blocks, counted per image
    assert lay.blk_off[0] == 0 and all(lay.blk_off[i + 1] - lay.blk_off[i] == -(-(h * w) // 256) for i, (h, w) in enumerate(sizes))
    # the patch list: image-major, every image's own grid in ddim_sample's order, spans back to back
    want = []
    for i, (h, w) in enumerate(sizes):
        hl, wl = sampling.overlapping_grid_indices(h, w, p, r)
        want += [(i, a, b) for a in hl for b in wl]
    assert list(lay.patches) == want and lay.n == len(want) and sum(lay.patch_counts) == lay.n
    for i, (h, w, lo, hi) in enumerate(lay.img_tab):
        assert (h, w) == sizes[i] and hi - lo == lay.patch_counts[i] and lo == sum(lay.patch_counts[:i])
        assert all(t[0] == i for t in lay.patches[lo:hi])
        assert all(0 <= a and a + p <= h and 0 <= b and b + p <= w for (_, a, b) in lay.patches[lo:hi])


def test_layout_views_are_the_images_blocks():
    import torch
    lay = sampling.RaggedLayout(THREE, 16, 4)
    for C in (3, 48):
        flat = torch.arange(lay.numel(C), dtype=torch.float32)
        seen = 0
        for i, (h, w) in enumerate(THREE):
            v = lay.view(flat, C, i)
            assert tuple(v.shape) == (1, C, h, w) and v.is_contiguous() and v.data_ptr() == flat.data_ptr() + 4 * C * lay.pix_off[i]
            assert float(v.reshape(-1)[0]) == seen and float(v.reshape(-1)[-1]) == seen + C * h * w - 1
            seen += C * h * w
        assert seen == flat.numel()


def test_layout_from_an_explicit_patch_list():
    lay = sampling.RaggedLayout.from_patches(FIVE, 16, [(0, 0, 0), (2, 0, 0), (2, 12, 0), (3, 4, 20)])
    assert lay.patch_counts == (1, 0, 2, 1, 0) and [t[2:] for t in lay.img_tab] == [(0, 1), (1, 1), (1, 3), (3, 4), (4, 4)]


def test_layout_refusals():
    with pytest.raises(ValueError, match="smaller than one"):
        sampling.RaggedLayout([(16, 16), (15, 16)], 16)
    with pytest.raises(ValueError, match="smaller than one"):
        sampling.RaggedLayout([(16, 12)], 16)
    with pytest.raises(ValueError, match="multiple of 4"):
        sampling.RaggedLayout([(16, 16), (16, 18)], 16)
    with pytest.raises(ValueError, match="not image-major"):
        sampling.RaggedLayout.from_patches(FIVE, 16, [(1, 0, 0), (0, 0, 0)])
    with pytest.raises(ValueError, match="leaves its"):
        sampling.RaggedLayout.from_patches(FIVE, 16, [(0, 0, 0), (1, 0, 5)])          # 5 + 16 > 20
    with pytest.raises(ValueError, match="leaves its"):
        sampling.RaggedLayout.from_patches(FIVE, 16, [(0, -1, 0)])
    with pytest.raises(ValueError, match="names image"):
        sampling.RaggedLayout.from_patches(FIVE, 16, [(5, 0, 0)])
    with pytest.raises(ValueError):
        sampling.RaggedLayout([], 16)
    with pytest.raises(ValueError):
        sampling.RaggedLayout.from_patches(FIVE, 16, [])


def _groups(counts, max_batch, images_per_call=None):
    """The feeder's loop over mix_group_step, without its threads."""
    groups, cur = [], []
    for c in counts:
        before, after = restoration.mix_group_step(cur, c, max_batch, images_per_call)
        if before and cur:
            groups.append(cur)
            cur = []
        cur = cur + [c]
        if after:
            groups.append(cur)
            cur = []
    if cur:
        groups.append(cur)
    return groups


def test_grouping_rule():
    # an explicit count: N images whatever their sizes
    assert _groups([8, 300, 45, 1, 1, 700, 2], 384, 3) == [[8, 300, 45], [1, 1, 700], [2]]
    assert _groups([8, 300, 45], 384, 1) == [[8], [300], [45]]
    # automatic: closed when the next image would push the patches over max_batch
    assert _groups([8, 45, 300, 31, 1, 384, 383, 2], 384) == [[8, 45, 300, 31], [1], [384], [383], [2]]
    assert _groups([100, 100, 100, 84, 1], 384, "auto") == [[100, 100, 100, 84], [1]]
    # an image of more patches than max_batch is a group of its own
    assert _groups([8, 500, 8, 8], 384) == [[8], [500], [8, 8]]
    assert _groups([500, 500], 384, 0) == [[500], [500]]
    assert restoration.mix_group_step([8], 500, 384) == (True, True) and restoration.mix_group_step([], 500, 384) == (False, True)
    # the cap of 64 images
    assert restoration.MIX_MAX_IMAGES == 64
    assert [len(g) for g in _groups([1] * 150, 384)] == [64, 64, 22]
    assert restoration.mix_group_step([1] * 62, 1, 384) == (False, False) and restoration.mix_group_step([1] * 63, 1, 384) == (False, True)
    # a pure function: the inputs are not changed
    counts = [8, 45]
    restoration.mix_group_step(counts, 300, 384)
    assert counts == [8, 45]


def _same_size_groups(shapes, limit):
    """The feeder's loop over _same_size_group_step, without its threads; an empty group would show up as such."""
    groups, cur = [], []
    for s in shapes:
        before, after = restoration._same_size_group_step(cur, s, limit(s) if callable(limit) else limit)
        if before:
            groups.append(cur)
            cur = []
        cur = cur + [s]
        if after:
            groups.append(cur)
            cur = []
    if cur:
        groups.append(cur)
    return groups


def test_same_size_grouping_rule():
    big, odd = (1, 6, 96, 112), (1, 6, 64, 80)
    step = restoration._same_size_group_step
    # a different shape closes the open group before the image joins; nothing is open: nothing to close
    assert step([big, big], odd, 8) == (True, False) and step([big, big], big, 8) == (False, False) and step([], odd, 8) == (False, False)
    # the limit-th image closes its group after it joined -- also when it has just opened the group
    assert step([big] * 6, big, 8) == (False, False) and step([big] * 7, big, 8) == (False, True)
    assert step([], big, 1) == (False, True) and step([big], odd, 1) == (True, True) and step([big], odd, 2) == (True, False)
    assert step([], big, 0) == (False, True)                                     # a group holds at least one image
    # the sequence of tests/test_gpu_io.py: seven 96x112 images, one 64x80 inserted at index 4, limit 8 -> 4, 1, 3
    seq = [big] * 7
    seq.insert(4, odd)
    assert _same_size_groups(seq, 8) == [[big] * 4, [odd], [big] * 3]
    assert [len(g) for g in _same_size_groups(seq, 2)] == [2, 2, 1, 2, 1] and [len(g) for g in _same_size_groups(seq, 1)] == [1] * 8
    # a limit per size (images_per_call_for of the item's own size): the item's limit is its group's
    assert [len(g) for g in _same_size_groups(seq, lambda s: 3 if s == big else 1)] == [3, 1, 1, 3]
    # never an empty group, every image exactly once and in order, whatever the shapes and the limit
    for limit in (1, 2, 3, 8):
        for shapes in ([], [big], [odd, big], seq, [big, odd] * 4, [odd] * 9):
            groups = _same_size_groups(shapes, limit)
            assert all(groups) and [s for g in groups for s in g] == shapes
            assert all(len(set(g)) == 1 and len(g) <= limit for g in groups)
    # a pure function: the inputs are not changed; lists compare like tuples (torch.Size is a tuple)
    open_ = [big, big]
    step(open_, odd, 8)
    assert open_ == [big, big] and step([list(big)], big, 8) == (False, False)


def test_folder_patch_count_is_the_padded_grid():
    assert restoration.folder_patch_count(70, 93, 16, 4) == 2 * 3              # padded to 80 x 96: 20 x 24 in the wavelet domain
    assert restoration.folder_patch_count(33, 40, 16, 4) == 1                  # smaller than one patch: padded to 64 x 64
    assert restoration.folder_patch_count(480, 720, 64, 16) == 45


EST = dict(max_batch=32, dtype="f32", r=4, steps=6)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mixed_estimate_equals_the_plain_one_for_equal_sizes(dtype):
    cfg = P.reduced_config()
    kw = dict(EST, dtype=dtype)
    for (h, w) in ((70, 93), (33, 40), (100, 130), (300, 300)):
        for n in (1, 2, 3, 7):
            assert restoration.estimate_restore_bytes_mixed([(h, w)] * n, cfg, **kw) == restoration.estimate_restore_bytes(h, w, n, cfg, **kw), (h, w, n)
    cfg48 = P.pred_channels_config(48)                                          # every band diffused: no HFRM term
    assert restoration.estimate_restore_bytes_mixed([(70, 93)] * 2, cfg48, **EST) == restoration.estimate_restore_bytes(70, 93, 2, cfg48, **EST)


def test_mixed_estimate_is_non_decreasing():
    cfg = P.reduced_config()
    est = lambda sizes: restoration.estimate_restore_bytes_mixed(sizes, cfg, **EST)
    folder = [(70, 93), (64, 64), (96, 112), (33, 40), (70, 93)]
    # an image added
    for k in range(1, len(folder)):
        assert est(folder[:k]) < est(folder[:k + 1])
    assert est(folder) <= est(folder + [(1, 1)])
    # an image enlarged, in either direction, also out of a run of equal sizes
    hs = [1, 17, 64, 65, 70, 80, 81, 130, 300]
    for a, b in zip(hs, hs[1:]):
        assert est([(70, 93), (a, 93), (70, 93)]) <= est([(70, 93), (b, 93), (70, 93)])
        assert est([(70, 93), (70, a), (70, 93)]) <= est([(70, 93), (70, b), (70, 93)])
    assert est([(70, 93), (70, 93)]) <= est([(70, 93), (70, 97)]) <= est([(81, 93), (70, 97)])
    # a mixed call needs more than its largest image alone
    assert est(folder) > max(restoration.estimate_restore_bytes(h, w, 1, cfg, **EST) for (h, w) in folder)
    with pytest.raises(ValueError):
        est([])
