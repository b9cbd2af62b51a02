"""Host-side parts of the HFRM trainer's mixed precision (no GPU): the dtype name, wdm_hfrm_trainer_set_precision on a host-only trainer
-- workspace sizes against tests/golden/layout.json, the parameter table, the refusals -- and the sample sheet against a numpy
restatement of the reference's sample_images."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from wavedm_amd import _lib
from wavedm_amd.hfrm_training import MIXED, _resolve_train_dtype, sample_sheet

HFRM_CFGS = {"default": dict(mid=6, enc=(2, 2, 2, 4), dec=(2, 2, 2, 2)), "small": dict(mid=1, enc=(1, 1), dec=(1, 1))}
SHAPES = ((64, 64), (96, 160))


def _trainer(k):
    c = _lib.HFRMConfig()
    c.in_channel, c.dim, c.mid_blk_num, c.n_enc, c.n_dec, c.dtype = 3, 32, k["mid"], len(k["enc"]), len(k["dec"]), _lib.WDM_F32
    for i, v in enumerate(k["enc"]):
        c.enc_blk_nums[i] = v
    for i, v in enumerate(k["dec"]):
        c.dec_blk_nums[i] = v
    t = C.c_void_p()
    _lib.check(_lib.lib().wdm_hfrm_trainer_create(None, C.byref(c), C.byref(t)))
    return t


def _params(t):
    L = _lib.lib()
    name, ndim, shape, off = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int64()
    rows = []
    for i in range(L.wdm_hfrm_trainer_num_params(t)):
        _lib.check(L.wdm_hfrm_trainer_param_info(t, i, C.byref(name), C.byref(ndim), C.byref(shape), C.byref(off)))
        rows.append([name.value.decode(), [int(shape[k]) for k in range(ndim.value)], int(off.value)])
    return rows


def _workspace(t):
    return {f"1x{h}x{w}": int(_lib.lib().wdm_hfrm_trainer_workspace_bytes(t, 1, h, w)) for h, w in SHAPES}


def test_dtype_names():
    assert MIXED == "bf16-mixed" and MIXED not in _lib.DTYPES
    assert _resolve_train_dtype("bf16-mixed") == _lib.WDM_BF16
    for name in (None, "f32", "f16", "f32x3"):
        assert _resolve_train_dtype(name) == _lib.WDM_F32
    with pytest.raises(NotImplementedError, match="bf16-mixed"):
        _resolve_train_dtype("bf16")
    with pytest.raises(ValueError):
        _resolve_train_dtype("f64")


@pytest.mark.parametrize("cname", sorted(HFRM_CFGS))
def test_set_precision_on_host_trainer(cname):
    L = _lib.lib()
    want = json.load(open(os.path.join(REPO, "tests", "golden", "layout.json")))["hfrm"][f"{cname}/f32"]["trainer"]
    t = _trainer(HFRM_CFGS[cname])
    try:
        assert _workspace(t) == want["workspace_bytes"]                     # the state after create is WDM_F32
        rows32, n32 = _params(t), int(L.wdm_hfrm_trainer_num_floats(t))
        assert hashlib.sha256(json.dumps(rows32).encode()).hexdigest() == want["params"]["sha256"] and n32 == want["num_floats"]
        assert L.wdm_hfrm_trainer_set_precision(t, _lib.WDM_BF16) == _lib.WDM_OK
        mixed = _workspace(t)
        for k, v in mixed.items():
            assert 0 < v < want["workspace_bytes"][k], (k, v)
        assert _params(t) == rows32 and int(L.wdm_hfrm_trainer_num_floats(t)) == n32
        # refused settings leave the mode as it was, each with its reason
        assert L.wdm_hfrm_trainer_set_precision(t, _lib.WDM_F16) == _lib.WDM_EINVAL
        msg = L.wdm_last_error().decode()
        assert "fp16" in msg and "loss scaling" in msg and "exponent range" in msg
        assert L.wdm_hfrm_trainer_set_precision(t, _lib.WDM_F32X3) == _lib.WDM_EINVAL
        assert L.wdm_hfrm_trainer_set_precision(t, 17) == _lib.WDM_EINVAL
        assert "unsupported" in L.wdm_last_error().decode()
        assert _workspace(t) == mixed
        assert L.wdm_hfrm_trainer_set_precision(t, _lib.WDM_F32) == _lib.WDM_OK
        assert _workspace(t) == want["workspace_bytes"]
        assert _params(t) == rows32
    finally:
        L.wdm_hfrm_trainer_destroy(t)
    assert L.wdm_hfrm_trainer_set_precision(None, _lib.WDM_BF16) == _lib.WDM_EINVAL


def test_config_dtype_does_not_select_the_mode():
    """The mode is a setting of the trainer, not of wdm_hfrm_config: create still refuses every dtype but WDM_F32."""
    L = _lib.lib()
    for code in (_lib.WDM_BF16, _lib.WDM_F16, _lib.WDM_F32X3):
        c = _lib.HFRMConfig()
        c.in_channel, c.dim, c.mid_blk_num, c.n_enc, c.n_dec, c.dtype = 3, 32, 1, 1, 1, code
        c.enc_blk_nums[0] = c.dec_blk_nums[0] = 1
        t = C.c_void_p()
        assert L.wdm_hfrm_trainer_create(None, C.byref(c), C.byref(t)) == _lib.WDM_EINVAL


def _sheet_numpy(inp, out, gt):
    """train_hfrm.py's sample_images in numpy: x * 255 in fp32, the prediction clamped to [0, 255], .int() = truncation toward zero."""
    data = (inp[0].numpy().astype(np.float32) * np.float32(255))
    pred = np.clip(out[0].numpy().astype(np.float32) * np.float32(255), np.float32(0), np.float32(255))
    label = (gt[0].numpy().astype(np.float32) * np.float32(255))
    h, w = pred.shape[-2:]
    img = np.zeros((h, 3 * w, 3))
    for k, t in enumerate((data, pred, label)):
        img[:, k * w:(k + 1) * w] = np.transpose(np.trunc(t).astype(np.int32), (1, 2, 0))
    return img.astype(np.uint8)


def test_sample_sheet_matches_numpy():
    g = torch.Generator().manual_seed(7)
    inp = torch.rand(2, 3, 10, 14, generator=g)
    gt = torch.rand(2, 3, 10, 14, generator=g)
    out = torch.rand(2, 3, 10, 14, generator=g) * 1.6 - 0.3             # predictions outside [0, 1] on both sides
    edge = torch.tensor([0.999, 0.9999999, 1.0, 0.0, 1 / 255, 2 / 255 - 1e-7, 254.9999 / 255, 0.5, 0.00392, 0.99607843])
    inp[0, 0, 0, :10] = edge
    gt[0, 1, 3, :10] = edge
    out[0, 2, 5, :10] = edge
    out[0, 0, 1, :4] = torch.tensor([-0.5, 1.5, 1.0000001, -1e-9])
    sheet = sample_sheet(inp, out, gt)
    assert sheet.dtype == torch.uint8 and tuple(sheet.shape) == (10, 42, 3) and sheet.is_contiguous()
    want = _sheet_numpy(inp, out, gt)
    assert np.array_equal(sheet.numpy(), want)
    assert int(sheet[0, 0, 0]) == 254 and int(sheet[0, 2, 0]) == 255       # 0.999 * 255 = 254.745 truncates (rounding would give 255)
    assert sheet[1, 14:18, 0].tolist() == [0, 255, 255, 0]
    assert not np.array_equal(sheet.numpy(), _sheet_numpy(inp[1:], out[1:], gt[1:]))      # batch element 0, not 1
