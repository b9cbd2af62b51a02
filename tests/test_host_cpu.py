"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol the header declares,
the parameter table equals the reference's state_dict layout, host-side sampler arithmetic, fail-loud behaviour."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from wavedm_amd import _lib
from wavedm_amd import procedural as P
from oracle import wavedm_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(REPO, "include", "wavedm.h")).read()
    declared = sorted(set(re.findall(r"\b(wdm_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 24
    L = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/wavedm.h but not exported"
    assert sorted(_lib.EXPORTED) == declared
    assert _lib.lib().wdm_abi_version() == 1


def test_ctypes_signatures_agree_with_the_header():
    """Every prototype of include/wavedm.h against the ctypes binding: same number of arguments, same kind (pointer / int / float /
    size_t / int64) in the same order, same return kind -- a silent mismatch here would corrupt arguments instead of failing."""
    hdr = open(os.path.join(REPO, "include", "wavedm.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(wdm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr)
    assert len(protos) == len(_lib.EXPORTED)

    def kind_c(decl, is_param=True):
        decl = decl.strip()
        if decl in ("void", ""):
            return None
        if "*" in decl or "[" in decl:
            return "ptr"
        words = re.sub(r"\b(const|unsigned|extern|WDM_API)\b", "", decl).split()
        ty = " ".join(words[:-1]) if (is_param and len(words) > 1) else " ".join(words)
        return {"int": "int", "float": "float", "size_t": "size_t", "int64_t": "i64", "double": "double"}[ty]

    def kind_py(a):
        if a is None:
            return None
        if a in (C.c_void_p, C.c_char_p) or (isinstance(a, type) and issubclass(a, C._Pointer)):
            return "ptr"
        return {C.c_int: "int", C.c_float: "float", C.c_size_t: "size_t", C.c_int64: "i64", C.c_double: "double"}[a]

    L = _lib.lib()
    for ret, name, params in protos:
        fn = getattr(L, name)
        want = [k for k in (kind_c(x) for x in params.split(",")) if k]
        assert [kind_py(a) for a in fn.argtypes] == want, name
        assert kind_py(fn.restype) == kind_c(ret, is_param=False), name


@pytest.mark.parametrize("cfg", [P.raindrop_wavelet_config(), P.reduced_config(), P.raindrop_wavelet_config(image_size=128)])
def test_param_table_matches_reference_state_dict_layout(cfg):
    import wavedm_amd
    net = wavedm_amd.DiffusionUNet(cfg, dtype="bf16")
    sd = net.state_dict()
    ref = P.unet_param_shapes(cfg)
    assert set(sd) == set(ref)
    assert all(tuple(sd[k].shape) == tuple(ref[k]) for k in ref)
    net.load_state_dict(P.procedural_state_dict(cfg) if cfg.model.ch == 32 else sd, strict=True)
    assert net.module is net
    assert net.packed_bytes() > sum(v.numel() for v in sd.values()) * 2 * 0.99
    # workspace query is a pure host computation
    assert int(_lib.lib().wdm_unet_workspace_bytes(net._u, 4)) > 0


@pytest.mark.parametrize("kind", P.VARIANTS)
def test_optional_branch_param_tables(golden, kind):
    """The optional config branches change conv_in / conv_out widths and (wavelet_in_unet) add two frozen Haar weights."""
    import wavedm_amd
    cfg, _ = P.variant_config(kind)
    net = wavedm_amd.DiffusionUNet(cfg, dtype="f32")
    sd = net.state_dict()
    frozen = [k for k in sd if k.startswith("wavelet_")]
    want = P.unet_param_shapes(cfg)
    assert {k for k in sd if k not in frozen} == set(want.keys())
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    assert tuple(sd["conv_in.weight"].shape)[1] == P.unet_in_channels(cfg) == {"no_other": 51, "window": 24, "wavelet_in_unet": 96}[kind]
    v = golden("variants.npz")
    assert frozen == (["wavelet_dec.conv.weight", "wavelet_rec.conv.weight"] if kind == "wavelet_in_unet" else [])
    for k in frozen:                                            # same values as the reference un-pickles
        assert np.array_equal(sd[k].numpy(), v[kind + ":" + k]) and not dict(net.named_parameters())[k].requires_grad
    full = dict(P.procedural_state_dict(cfg, seed=61), **{k: torch.from_numpy(v[kind + ":" + k]) for k in frozen})
    net.load_state_dict(full, strict=True)


def test_no_cpu_fallback():
    import wavedm_amd
    with pytest.raises(TypeError):
        wavedm_amd.WaveletTransform(scale=2, dec=True)(torch.zeros(1, 3, 8, 8))          # CPU tensor -> refuse
    net = wavedm_amd.DiffusionUNet(P.reduced_config())
    with pytest.raises((TypeError, RuntimeError)):
        net(torch.zeros(1, 96, 16, 16), torch.zeros(1))
    with pytest.raises(NotImplementedError):
        wavedm_amd.WaveletTransform(scale=1, dec=True)


def test_bad_arguments_return_errors_not_crashes():
    L = _lib.lib()
    cfg = _lib.UNetConfig()
    cfg.ch, cfg.n_levels, cfg.num_res_blocks, cfg.in_channels, cfg.out_ch, cfg.resolution = 30, 2, 2, 96, 3, 16
    cfg.ch_mult[0], cfg.ch_mult[1], cfg.resamp_with_conv, cfg.dtype = 1, 2, 1, 1
    u = C.c_void_p()
    assert L.wdm_unet_create(None, C.byref(cfg), C.byref(u)) == -1                           # ch % 32 != 0
    assert b"multiple of 32" in L.wdm_last_error()
    cfg.ch, cfg.resolution = 32, 12
    assert L.wdm_unet_create(None, C.byref(cfg), C.byref(u)) == -1                           # 12/2 = 6 not a multiple of 8
    cfg.resolution = 16
    assert L.wdm_unet_create(None, C.byref(cfg), C.byref(u)) == 0
    assert L.wdm_unet_load_param(u, b"conv_in.weight", C.c_void_p(16), 1, None) == -4        # no packed buffer yet
    assert L.wdm_unet_forward(u, C.c_void_p(16), C.c_void_p(16), 1, 1, C.c_void_p(16), C.c_void_p(256), 1 << 20, None) == -4
    L.wdm_unet_destroy(u)


def test_sampler_host_arithmetic_matches_oracle():
    from oracle import wavedm_oracle as O
    from wavedm_amd import sampling
    cfg = P.raindrop_wavelet_config()
    b = torch.from_numpy(sampling.get_beta_schedule("linear", beta_start=1e-4, beta_end=0.02, num_diffusion_timesteps=1000)).float()
    assert torch.equal(b, O.beta_schedule(cfg))
    tab = sampling.alpha_bar_table(b)
    for t in (-1, 0, 10, 500, 990, 999):
        assert float(tab[t + 1]) == float(O.compute_alpha(b, t))
        assert float(sampling.compute_alpha(b, torch.tensor([t])).flatten()[0]) == float(O.compute_alpha(b, t))
    for (h, w, p, r) in [(64, 64, 64, 16), (120, 180, 64, 16), (65, 70, 64, 16), (30, 45, 16, 4)]:
        assert sampling.overlapping_grid_indices(h, w, p, r) == O.overlapping_grid_indices(h, w, p, r)


def test_hfrm_param_table_matches_reference_state_dict_layout():
    """wdm_hfrm_param_info enumerates the reference HFRM's state_dict keys in registration order (arch.py:206-233)."""
    from wavedm_amd.arch import HFRM
    m = HFRM(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=[2, 2, 2, 4], dec_blk_nums=[2, 2, 2, 2])
    want = P.hfrm_param_shapes()
    sd = m.state_dict()
    assert list(sd.keys()) == list(want.keys())
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    assert sum(v.numel() for v in sd.values()) == 15941667
    with pytest.raises(RuntimeError):
        m.pack_weights()              # CPU parameters: no CPU path


def test_raindrop_dataset_matches_reference_golden(golden, tmp_path):
    """datasets/raindrop.py eval path (PIL LANCZOS to 720x480, multiples of 16, ToTensor) -- same items as the reference class
    produced on the same synthetic PNGs when the golden file was written."""
    import random
    from wavedm_amd.datasets import RainDropDataset, eval_size
    g = golden("io.npz")
    O.synthetic_raindrop_dir(str(tmp_path), seed=303)
    random.seed(61)
    ds = RainDropDataset(dir=str(tmp_path / "raindrop" / "raindrop_test"), patch_size=256, n=8, parse_patches=False)
    assert len(ds) == 3
    assert [ds[i][1] for i in range(3)] == [str(v) for v in g["ds_order"]]
    for i in range(3):
        x, img_id, total = ds[i]
        assert tuple(x.shape) == tuple(g[f"ds_{img_id}_shape"])
        assert np.array_equal(x.flatten()[::997].numpy(), g[f"ds_{img_id}_sub"])
        assert abs(float(x.double().sum()) - float(g[f"ds_{img_id}_sum"])) < 1e-6 * float(g[f"ds_{img_id}_sum"])
        assert torch.equal(total, x[:3])
    assert eval_size(720, 480) == (720, 480) and eval_size(2000, 1000) == (1024, 512) and eval_size(500, 1500) == (352, 1024)
    assert eval_size(721, 481) == (736, 496)
    # training path: n crops of patch_size, same crop for input and ground truth
    random.seed(5)
    dt = RainDropDataset(dir=str(tmp_path / "raindrop" / "raindrop_test"), patch_size=64, n=4, parse_patches=True)
    x, img_id, total = dt[0]
    assert tuple(x.shape) == (4, 6, 64, 64) and tuple(total.shape) == (4, 3, 480, 720)


def test_raindrop_loaders_use_a_fork_server_and_keep_their_workers(tmp_path):
    """RainDrop.get_loaders with num_workers > 0: worker processes from a fork server (forked children of a process with a HIP context slow its launches tenfold,
    datasets.worker_kwargs), alive across passes; the items are the ones the in-process loader gives, pass after pass."""
    import random
    from types import SimpleNamespace
    from wavedm_amd.datasets import RainDrop, worker_kwargs
    O.synthetic_raindrop_dir(str(tmp_path), seed=303)
    for leaf in ("input", "gt"):
        os.makedirs(tmp_path / "raindrop" / "train" / leaf)
    got = {}
    for nw in (0, 2):
        cfg = P.reduced_config()
        cfg.data.data_dir, cfg.data.num_workers = str(tmp_path), nw
        cfg.training = SimpleNamespace(patch_n=2, batch_size=1)
        random.seed(3)
        _, val = RainDrop(SimpleNamespace(world_size=1, rank=0), cfg).get_loaders(parse_patches=False, validation="raindrop")
        if nw:
            assert val.multiprocessing_context.get_start_method() == "forkserver" and val.persistent_workers
        got[nw] = [[(y[0], float(x.double().sum()), tuple(x.shape)) for x, y, t in val] for _ in range(2)]
    assert got[0][0] == got[2][0] == got[2][1] and len(got[0][0]) == 3
    cfg.data.worker_context = "fork"
    assert worker_kwargs(cfg, 2) == {} and worker_kwargs(P.reduced_config(), 0) == {}


def test_trainer_param_table_on_host():
    """wdm_trainer_param_info needs no GPU: every state_dict entry of the reference once, offsets tile the flat buffer exactly."""
    from wavedm_amd.unet import _make_config
    L = _lib.lib()
    for cfg in (P.reduced_config(), P.raindrop_wavelet_config()):
        c = _make_config(cfg, _lib.WDM_BF16)
        t = C.c_void_p()
        _lib.check(L.wdm_trainer_create(None, C.byref(c), C.byref(t)))
        name, ndim, shape, off = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int64()
        want = P.unet_param_shapes(cfg)
        seen, spans = {}, []
        for i in range(L.wdm_trainer_num_params(t)):
            _lib.check(L.wdm_trainer_param_info(t, i, C.byref(name), C.byref(ndim), C.byref(shape), C.byref(off)))
            shp = tuple(int(shape[k]) for k in range(ndim.value))
            seen[name.value.decode()] = shp
            spans.append((int(off.value), int(np.prod(shp))))
        assert seen == {k: tuple(v) for k, v in want.items()}
        spans.sort()
        assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:]))
        assert spans[-1][0] + spans[-1][1] == int(L.wdm_trainer_num_floats(t)) == sum(int(np.prod(v)) for v in want.values())
        L.wdm_trainer_destroy(t)


def test_make_grid_matches_torchvision_layout():
    """imageio.make_grid against the oracle's restatement of torchvision.utils.make_grid (validation sheet, ddm_wavelet.py:407-410)."""
    from wavedm_amd.imageio import make_grid
    g = torch.Generator().manual_seed(3)
    for (n, c, h, w, nrow, pad) in [(8, 3, 12, 20, 4, 2), (5, 3, 7, 9, 4, 2), (1, 3, 6, 6, 4, 2), (3, 1, 5, 4, 8, 1), (4, 3, 8, 8, 4, 0)]:
        t = torch.rand(n, c, h, w, generator=g)
        a, b = make_grid(t, nrow=nrow, padding=pad), O.make_grid(t, nrow=nrow, padding=pad)
        assert a.shape == b.shape and torch.equal(a, b)
    assert tuple(make_grid(torch.rand(8, 3, 12, 20), nrow=4).shape) == (3, 2 * 14 + 2, 4 * 22 + 2)


def test_config_file_matches_reference_yaml(golden):
    """configs/raindrop_wavelet.yml (and procedural.raindrop_wavelet_config()) carry every key of the reference's YAML with the same
    values: the canonical JSON hashes to the value recorded when the golden files were generated from the reference's file."""
    import hashlib
    import json
    from wavedm_amd.config import load_config, namespace2dict, dict2namespace
    g = golden("config.npz")
    shipped = namespace2dict(load_config(os.path.join(REPO, "configs", "raindrop_wavelet.yml")))
    built = namespace2dict(P.raindrop_wavelet_config())
    for d in (shipped, built):
        d["data"]["data_dir"], d["data"]["num_workers"] = "/data1/weather/", 32         # the reference file's deployment settings
        assert sorted(d) == [str(v) for v in g["sections"]] and sum(len(v) for v in d.values()) == int(g["n_keys"])
        assert hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest() == str(g["sha256"])
    ns = dict2namespace(shipped)
    assert ns.model.ch_mult == [1, 2, 4, 6] and ns.optim.lr == 4e-5 and ns.training.patch_n == 8 and ns.data.wavelet is True


def test_parameter_order_is_the_references(golden):
    """torch.optim state dicts index parameters by position (ddm_wavelet.py:186, :288), so `named_parameters()` must walk the tree in the
    reference's order.  tests/golden/train.npz holds the reference's own `named_parameters()` key order for the reduced model."""
    import wavedm_amd
    from wavedm_amd import procedural as P
    want = [str(k) for k in golden("train.npz")["grad_names"]]
    m = wavedm_amd.DiffusionUNet(P.reduced_config(), dtype="f32")
    assert [k for k, _ in m.named_parameters()] == want
    # from-scratch initialisation follows nn.Conv2d / nn.Linear reset_parameters: biases are uniform(+-1/sqrt(fan_in)), not zero
    sd = dict(m.named_parameters())
    b = sd["down.0.block.0.conv1.bias"]
    bound = 1.0 / (sd["down.0.block.0.conv1.weight"][0].numel() ** 0.5)
    assert float(b.abs().max()) <= bound and float(b.abs().max()) > 0.0
    assert float(sd["down.0.block.0.norm1.bias"].abs().max()) == 0.0 and float((sd["down.0.block.0.norm1.weight"] - 1).abs().max()) == 0.0


def test_f16_mode_layout_is_the_bf16_layout_plus_the_range_flag():
    """WDM_F16 (round 5): same packed layout and workspace as bf16 (2-byte elements, the same copies) plus one 256-byte slot for the weight loader's range flag;
    the HFRM and the trainer map the mode to f32; unknown dtype names are refused."""
    import wavedm_amd
    cfg = P.raindrop_wavelet_config()
    a, b = wavedm_amd.DiffusionUNet(cfg, dtype="bf16"), wavedm_amd.DiffusionUNet(cfg, dtype="f16")
    assert b._dtype_code == _lib.WDM_F16 and b._torch_dtype == torch.float16
    assert b.packed_bytes() == a.packed_bytes() + 256
    L = _lib.lib()
    assert int(L.wdm_unet_workspace_bytes(b._u, 8)) == int(L.wdm_unet_workspace_bytes(a._u, 8))
    from wavedm_amd.arch import HFRM
    assert HFRM(in_channel=3, dim=32, mid_blk_num=1, enc_blk_nums=[1], dec_blk_nums=[1], dtype="f16")._dtype_code == _lib.WDM_F32
    with pytest.raises(ValueError):
        wavedm_amd.DiffusionUNet(cfg, dtype="fp8")


def test_bench_dump_outputs_keeps_the_same_rows_under_its_budget(tmp_path):
    """bench.py --dump-outputs: float32 .npy files; outputs over 64 MB keep a fixed, seeded sample of their rows -- the same rows in every array
    and in every run, in order --, outputs under it are written whole."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    big = torch.arange(40, dtype=torch.float64).view(40, 1, 1, 1).expand(40, 3, 512, 512)       # 126 MB in float32, row k holds k
    small = torch.arange(40 * 8, dtype=torch.float32).reshape(40, 8)
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), {"big": big, "small": small, "absent": None})
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("big", "small")}
    assert all(np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy")) for n in a)
    assert a["big"].dtype == a["small"].dtype == np.float32
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in a) <= 64 * 1000 * 1000
    rows = a["small"][:, 0] / 8
    assert 0 < len(rows) < 40 and np.all(np.diff(rows) > 0) and np.array_equal(a["small"], small.numpy()[rows.astype(int)])
    assert a["big"].shape == (len(rows), 3, 512, 512) and np.array_equal(a["big"], np.broadcast_to(rows.reshape(-1, 1, 1, 1), a["big"].shape))
    bench.dump_outputs(str(tmp_path / "c"), {"small": small})
    assert np.array_equal(np.load(tmp_path / "c" / "small.npy"), small.numpy())


def _layout_table():
    """Everything the host-side model descriptions decide, as plain integers and strings: parameter enumerations (the trainers' with offsets), packed / workspace
    sizes, per config and dtype.  Full-size configs keep one SHA-256 per enumeration beside the totals."""
    import hashlib
    import json
    from wavedm_amd.config import load_config
    from wavedm_amd.unet import _make_config
    L = _lib.lib()
    name, ndim, shape, off = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int64()

    def enum(n, info, obj, with_off):
        rows = []
        for i in range(n):
            _lib.check(info(obj, i, C.byref(name), C.byref(ndim), C.byref(shape), *([C.byref(off)] if with_off else [])))
            rows.append([name.value.decode(), [int(shape[k]) for k in range(ndim.value)]] + ([int(off.value)] if with_off else []))
        return rows

    def listed(rows, full):
        out = {"n": len(rows), "sha256": hashlib.sha256(json.dumps(rows).encode()).hexdigest()}
        if full:
            out["rows"] = rows
        return out

    dtypes = (("bf16", _lib.WDM_BF16), ("f16", _lib.WDM_F16), ("f32", _lib.WDM_F32), ("f32x3", _lib.WDM_F32X3))
    unet_cfgs = [("reduced", P.reduced_config()), ("raindrop", P.raindrop_wavelet_config()), ("raindrop128", P.raindrop_wavelet_config(image_size=128))]
    unet_cfgs += [(k, P.variant_config(k)[0]) for k in P.VARIANTS]
    unet_cfgs += [(k, load_config(os.path.join(REPO, "configs", f"raindrop_wavelet_{k}.yml"))) for k in ("pc12", "pc48")]
    table = {"unet": {}, "hfrm": {}}
    for cname, cfg in unet_cfgs:
        full = cname == "reduced"
        for dname, code in dtypes:
            c, u, e = _make_config(cfg, code), C.c_void_p(), {}
            e["create"] = int(L.wdm_unet_create(None, C.byref(c), C.byref(u)))
            if e["create"] == 0:
                e["params"] = listed(enum(L.wdm_unet_num_params(u), L.wdm_unet_param_info, u, False), full)
                e["packed_bytes"] = int(L.wdm_unet_packed_bytes(u))
                e["workspace_bytes"] = {str(B): int(L.wdm_unet_workspace_bytes(u, B)) for B in (1, 4)}
                e["temb_rows"] = int(L.wdm_unet_temb_rows(u))
                L.wdm_unet_destroy(u)
            t, tr = C.c_void_p(), {}
            tr["create"] = int(L.wdm_trainer_create(None, C.byref(c), C.byref(t)))
            if tr["create"] == 0:
                tr["params"] = listed(enum(L.wdm_trainer_num_params(t), L.wdm_trainer_param_info, t, True), full)
                tr["num_floats"] = int(L.wdm_trainer_num_floats(t))
                L.wdm_trainer_destroy(t)
            table["unet"][f"{cname}/{dname}"] = {"sampler": e, "trainer": tr}
    # the default HFRM and the smallest one both engines accept (they refuse any dim but the reference's 32): one block per level, two levels
    hfrm_cfgs = [("default", dict(mid=6, enc=(2, 2, 2, 4), dec=(2, 2, 2, 2))), ("small", dict(mid=1, enc=(1, 1), dec=(1, 1)))]
    for cname, k in hfrm_cfgs:
        full = cname == "small"
        for dname, code in dtypes:
            c = _lib.HFRMConfig()
            c.in_channel, c.dim, c.mid_blk_num, c.n_enc, c.n_dec, c.dtype = 3, 32, k["mid"], len(k["enc"]), len(k["dec"]), code
            for i, v in enumerate(k["enc"]):
                c.enc_blk_nums[i] = v
            for i, v in enumerate(k["dec"]):
                c.dec_blk_nums[i] = v
            m, e = C.c_void_p(), {}
            e["create"] = int(L.wdm_hfrm_create(None, C.byref(c), C.byref(m)))
            if e["create"] == 0:
                e["params"] = listed(enum(L.wdm_hfrm_num_params(m), L.wdm_hfrm_param_info, m, False), full)
                e["packed_bytes"] = int(L.wdm_hfrm_packed_bytes(m))
                e["workspace_bytes"] = {f"1x{h}x{w}": int(L.wdm_hfrm_workspace_bytes(m, 1, h, w)) for h, w in ((64, 64), (96, 160))}
                L.wdm_hfrm_destroy(m)
            t, tr = C.c_void_p(), {}
            tr["create"] = int(L.wdm_hfrm_trainer_create(None, C.byref(c), C.byref(t)))
            if tr["create"] == 0:
                tr["params"] = listed(enum(L.wdm_hfrm_trainer_num_params(t), L.wdm_hfrm_trainer_param_info, t, True), full)
                tr["num_floats"] = int(L.wdm_hfrm_trainer_num_floats(t))
                tr["workspace_bytes"] = {f"1x{h}x{w}": int(L.wdm_hfrm_trainer_workspace_bytes(t, 1, h, w)) for h, w in ((64, 64), (96, 160))}
                L.wdm_hfrm_trainer_destroy(t)
            table["hfrm"][f"{cname}/{dname}"] = {"sampler": e, "trainer": tr}
    return table


def test_model_layouts_are_the_recorded_ones():
    """Sampler and trainer of both networks enumerate the same parameters in the same order at the same offsets, and ask for the same packed and workspace
    bytes, as recorded in tests/golden/layout.json: the packed buffer is broadcast between ranks, the trainers' order is the checkpoint format.  The workspace
    queries dry-run the forward / training walks, so they also show that every layer record still reaches its consumer.  Integers and strings: equality.

    The file is `json.dump(_layout_table(), f, sort_keys=True, separators=(",", ":"))` run at commit 3290842 ("HFRM: local channel-attention pooling ..."),
    the last one whose engines each built their own layer list; the reduced UNet and the small HFRM are listed in full, the rest as a SHA-256 per list."""
    import json
    want = json.load(open(os.path.join(REPO, "tests", "golden", "layout.json")))
    got = json.loads(json.dumps(_layout_table()))
    assert sorted(got) == sorted(want)
    for net in want:
        assert sorted(got[net]) == sorted(want[net])
        for key in want[net]:
            assert got[net][key] == want[net][key], (net, key)
