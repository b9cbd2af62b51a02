"""Every attention core, through the C ABI (wdm_attn_forward), against the float64 reference on the operands the device rounds (attn_ref.py), on input families
that let the attention term -- not the residual -- set the output's rounding step (attn_ref.family).

16-bit outputs: fwd_ref.check16 -- |got - ref| <= 1 ulp16(ref) + F x M everywhere, at most a share S of the outputs off round16(ref).  fp32 outputs (f32, f32x3):
check32 -- |got - ref| <= C x 2^-24 x M.  Which core ran is read from the profiler for every case and selects the reference form (and, in f32x3, the product
form of every GEMM), so a dispatcher change cannot leave a form untested.

Bounds.  Nothing is tuned on the kernels: per group (form, family, kind) F = 4 x the F the host emulation needs (attn_ref.attn_block_emu: the same chain in fp32
on the CPU, over every case of the group; test_host_attn_ref.py re-measures it), the factor 4 -- two bits -- for the device's summation order and its exp2 / expf /
reciprocal; S = 2 x the emulation's share (at least 1e-3, never above 0.4); C likewise 4 x the emulation's.  NEED holds the emulation's values, the bounds are
computed from them below; `device` is the worst value measured on an MI355X over the group's cases (the kernels are deterministic).

The emulation's GroupNorm.  A first table came from ONE fp32 GroupNorm (torch's) and the device missed one bound of it: fused, locator, bf16, C = 768 -- a share of
3.18e-3 against 2 x 1.12e-3.  There P is exactly 1 on a token's own key, O = V, and the only outputs off the rounded reference belong to the few tokens one of whose
hn fell on the other side of a 16-bit midpoint in GroupNorm: which tokens is an accident of the fp32 arithmetic (the device's is scale / shift fmas on fp64-reduced
statistics, gn_group.h), and one such token moves up to a third of its 768 outputs.  One draw of a count of one to five events is no yardstick: the emulation now
restates the device's GroupNorm and three other fp32 forms (attn_ref.GN_VARIANTS: 1.1e-3 to 3.5e-3 on that case) and the table takes the worst.  No kernel was
changed and the reference gained no rounding point.  (96 channels on 20 x 32 -- 640 tokens -- is refused by the GEMMs, whose maps are multiples of 8 both ways:
the 128-row query block runs on 16 x 40.)"""
import pytest
import torch

from attn_ref import attn_block_ref, family, permute_tokens
from fwd_ref import H16, check16, check32

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

K16 = ("bf16", "f16")
K32 = ("f32", "f32x3")
BASE = ("flat", "peaked", "locator", "large_logit")
FOLD0 = {"WDM_ATTN_FOLD": "0"}
STREAM0 = {"WDM_ATTN_STREAM": "0"}

# path, form, bound group, C, H, W, B, families, kinds, env
CASES = [
    # folded, one launch (QPROJ + PROJ): B 9 = one full group of 8 images and a ragged one; 384 is no power of two; 512 the PROJ limit
    ("folded1", "folded", "folded", 128, 16, 16, 9, BASE, K16, {}),
    ("folded1", "folded", "folded", 384, 16, 16, 2, BASE, K16, {}),
    ("folded1", "folded", "folded", 512, 16, 16, 2, BASE, K16, {}),
    # folded, projections outside: two phase-2 passes; 8 x 32 = 256 tokens that are no 16 x 16 map
    ("folded_ext", "folded", "folded", 768, 16, 16, 2, ("flat", "locator"), K16, {}),
    ("folded_ext", "folded", "folded", 1024, 16, 16, 1, ("flat", "locator"), K16, {}),
    ("folded_ext", "folded", "folded", 128, 8, 32, 2, ("flat", "locator"), K16, {}),
    # unfolded fused core: V by GEMM with its bias behind the softmax (256), channel-major V (128), two passes (768)
    ("fused", "fused", "fused", 256, 16, 16, 2, ("flat", "peaked", "locator"), K16, FOLD0),
    ("fused", "fused", "fused", 128, 16, 16, 2, ("flat", "peaked", "locator"), K16, FOLD0),
    ("fused", "fused", "fused", 768, 16, 16, 2, ("flat", "peaked", "locator"), K16, FOLD0),
    # block-diagonal 8 x 8: ragged last group, masking, one image alone
    ("bdiag", "folded", "bdiag", 128, 8, 8, 5, ("flat", "locator", "twins"), K16, {}),
    ("bdiag", "folded", "bdiag", 512, 8, 8, 1, ("flat", "locator", "twins"), K16, {}),
    ("bdiag", "folded", "bdiag", 768, 8, 8, 6, ("flat", "locator", "twins"), K16, {}),
    # three launches, 16-bit: softmax_rows_kernel at per = 4 (not fused-eligible), 1, 2, 3 and 8
    ("gemm3", "gemm", "gemm", 640, 16, 16, 2, BASE, K16, {}),
    ("gemm3", "gemm", "gemm", 64, 8, 8, 2, BASE, K16, {}),
    ("gemm3", "gemm", "gemm", 64, 8, 16, 2, BASE, K16, {}),
    ("gemm3", "gemm", "gemm", 96, 8, 24, 2, BASE, K16, {}),
    ("gemm3", "gemm", "gemm", 128, 16, 32, 2, BASE, K16, {}),
    # streaming core: nine key blocks; Q rows re-read above 768; the widest; the shipped model's top level
    ("stream", "stream", "stream", 128, 24, 24, 2, BASE, K16, {}),
    ("stream", "stream", "stream", 256, 32, 32, 1, ("flat", "locator"), K16, {}),
    ("stream", "stream", "stream", 896, 24, 24, 1, ("flat", "locator"), K16, {}),
    ("stream", "stream", "stream", 1024, 24, 24, 1, ("flat", "locator"), K16, {}),
    ("stream", "stream", "stream", 128, 64, 64, 1, ("locator",), K16, {}),
    # per query block: blocks of 64, 128 and 256 rows; softmax_rows_long_kernel; copy_token_rows
    ("blocked", "gemm", "gemm", 96, 24, 24, 2, ("flat", "locator"), K16, {}),
    ("blocked", "gemm", "gemm", 96, 16, 40, 2, ("flat", "locator"), K16, {}),
    ("blocked", "gemm", "gemm", 128, 32, 32, 2, ("flat", "locator"), K16, STREAM0),
    # f32 and f32x3 (256 on 16 x 16: V^T from the GEMM form in f32x3)
    ("gemm3", "gemm", "gemm", 128, 16, 16, 2, BASE, K32, {}),
    ("gemm3", "gemm", "gemm", 256, 16, 16, 2, BASE, K32, {}),
    ("gemm3", "gemm", "gemm", 64, 8, 8, 2, BASE, K32, {}),
    ("gemm3", "gemm", "gemm", 64, 16, 32, 2, BASE, K32, {}),
    ("blocked", "gemm", "gemm", 128, 24, 24, 1, BASE, K32, {}),
]
# token permutations (locator inputs): the 16-bit cores, one case each -- (path, form, group, C, H, W, B, env)
PERM_CASES = [
    ("folded1", "folded", "folded", 128, 16, 16, 2, {}),
    ("stream", "stream", "stream", 128, 24, 24, 2, {}),
    ("bdiag", "folded", "bdiag", 128, 8, 8, 5, {}),
]

# (group, family, kind): what the host emulation needs, worst over the cases of the group and the four fp32 GroupNorms (`python tests/test_host_attn_ref.py`
# prints this table) -- 16-bit: (F, share); fp32: C.  Behind it the bound that follows and the device's worst with the case it comes from.
NEED = {
    ('bdiag', 'flat', 'bf16'): (2.70e-04, 4.18e-02),      # bound F 1.08e-03, S 8.36e-02; device F 2.70e-04 (C128 8x8 B5), S 2.55e-02 (C512 8x8 B1)
    ('bdiag', 'flat', 'f16'): (3.13e-05, 1.30e-01),       # bound F 1.25e-04, S 2.60e-01; device F 3.13e-05 (C128 8x8 B5), S 8.09e-02 (C768 8x8 B6)
    ('bdiag', 'locator', 'bf16'): (7.60e-05, 1.46e-03),   # bound F 3.04e-04, S 2.92e-03; device F 7.60e-05 (bdiag reversed token order), S 1.40e-03 (C512 8x8 B1)
    ('bdiag', 'locator', 'f16'): (2.47e-05, 5.96e-03),    # bound F 9.88e-05, S 1.19e-02; device F 2.47e-05 (bdiag reversed token order), S 4.17e-03 (C768 8x8 B6)
    ('bdiag', 'twins', 'bf16'): (5.77e-05, 1.00e-02),     # bound F 2.31e-04, S 2.00e-02; device F 4.74e-05 (C512 8x8 B1), S 5.46e-03 (C512 8x8 B1)
    ('bdiag', 'twins', 'f16'): (2.88e-05, 1.50e-01),      # bound F 1.15e-04, S 3.00e-01; device F 4.49e-05 (C128 8x8 B5), S 6.97e-02 (C768 8x8 B6)
    ('folded', 'flat', 'bf16'): (1.61e-04, 3.44e-02),     # bound F 6.44e-04, S 6.88e-02; device F 1.54e-04 (C128 16x16 B9), S 1.76e-02 (C512 16x16 B2)
    ('folded', 'flat', 'f16'): (3.16e-05, 2.16e-01),      # bound F 1.26e-04, S 4.00e-01; device F 3.16e-05 (C128 16x16 B9), S 1.39e-01 (C1024 16x16 B1)
    ('folded', 'large_logit', 'bf16'): (3.08e-03, 9.71e-03),# bound F 1.23e-02, S 1.94e-02; device F 3.08e-03 (C128 16x16 B9), S 8.61e-03 (C384 16x16 B2)
    ('folded', 'large_logit', 'f16'): (8.52e-04, 4.74e-02),# bound F 3.41e-03, S 9.48e-02; device F 5.23e-04 (C128 16x16 B9), S 2.97e-02 (C512 16x16 B2)
    ('folded', 'locator', 'bf16'): (5.63e-05, 2.68e-03),  # bound F 2.25e-04, S 5.36e-03; device F 5.63e-05 (C384 16x16 B2), S 1.50e-03 (C1024 16x16 B1)
    ('folded', 'locator', 'f16'): (3.82e-05, 7.63e-03),   # bound F 1.53e-04, S 1.53e-02; device F 3.35e-05 (folded1 random token order), S 4.12e-03 (C1024 16x16 B1)
    ('folded', 'peaked', 'bf16'): (1.06e-03, 2.46e-02),   # bound F 4.24e-03, S 4.92e-02; device F 9.02e-04 (C128 16x16 B9), S 2.36e-02 (C384 16x16 B2)
    ('folded', 'peaked', 'f16'): (4.59e-04, 8.82e-02),    # bound F 1.84e-03, S 1.76e-01; device F 1.57e-04 (C128 16x16 B9), S 4.93e-02 (C512 16x16 B2)
    ('fused', 'flat', 'bf16'): (1.42e-04, 4.41e-02),      # bound F 5.68e-04, S 8.82e-02; device F 1.46e-04 (C128 16x16 B2), S 3.72e-02 (C768 16x16 B2)
    ('fused', 'flat', 'f16'): (2.14e-05, 2.97e-01),       # bound F 8.56e-05, S 4.00e-01; device F 1.69e-05 (C128 16x16 B2), S 2.39e-01 (C768 16x16 B2)
    ('fused', 'locator', 'bf16'): (1.39e-04, 3.52e-03),   # bound F 5.56e-04, S 7.04e-03; device F 1.39e-04 (C768 16x16 B2), S 3.18e-03 (C768 16x16 B2)
    ('fused', 'locator', 'f16'): (7.10e-05, 3.62e-02),    # bound F 2.84e-04, S 7.24e-02; device F 6.34e-05 (C128 16x16 B2), S 2.16e-02 (C768 16x16 B2)
    ('fused', 'peaked', 'bf16'): (9.48e-04, 3.93e-02),    # bound F 3.79e-03, S 7.86e-02; device F 6.43e-04 (C256 16x16 B2), S 3.45e-02 (C768 16x16 B2)
    ('fused', 'peaked', 'f16'): (2.93e-04, 2.06e-01),     # bound F 1.17e-03, S 4.00e-01; device F 1.42e-04 (C256 16x16 B2), S 1.40e-01 (C768 16x16 B2)
    ('gemm', 'flat', 'bf16'): (1.81e-04, 1.47e-01),       # bound F 7.24e-04, S 2.94e-01; device F 2.62e-04 (C96 16x40 B2), S 1.47e-01 (C640 16x16 B2)
    ('gemm', 'flat', 'f16'): (4.18e-05, 2.71e-01),        # bound F 1.67e-04, S 4.00e-01; device F 4.18e-05 (C96 16x40 B2), S 2.36e-01 (C640 16x16 B2)
    ('gemm', 'flat', 'f32'): 2.44,                        # bound C 10; device 2.5 (C64 8x8 B2)
    ('gemm', 'flat', 'f32x3'): 24.35,                     # bound C 97; device 28.2 (C64 8x8 B2)
    ('gemm', 'large_logit', 'bf16'): (2.23e-03, 1.12e-02),# bound F 8.92e-03, S 2.24e-02; device F 8.48e-04 (C128 16x32 B2), S 4.75e-03 (C640 16x16 B2)
    ('gemm', 'large_logit', 'f16'): (1.08e-03, 1.10e-01), # bound F 4.32e-03, S 2.20e-01; device F 2.26e-03 (C64 8x16 B2), S 7.15e-02 (C640 16x16 B2)
    ('gemm', 'large_logit', 'f32'): 181.92,               # bound C 728; device 211.5 (C64 16x32 B2)
    ('gemm', 'large_logit', 'f32x3'): 899.54,             # bound C 3598; device 712.0 (C64 16x32 B2)
    ('gemm', 'locator', 'bf16'): (2.71e-04, 1.94e-03),    # bound F 1.08e-03, S 3.88e-03; device F 1.76e-04 (C640 16x16 B2), S 1.86e-03 (C640 16x16 B2)
    ('gemm', 'locator', 'f16'): (1.05e-04, 3.14e-02),     # bound F 4.20e-04, S 6.28e-02; device F 1.05e-04 (C96 24x24 B2), S 1.81e-02 (C640 16x16 B2)
    ('gemm', 'locator', 'f32'): 8.64,                     # bound C 35; device 8.6 (C64 16x32 B2)
    ('gemm', 'locator', 'f32x3'): 87.90,                  # bound C 352; device 73.1 (C64 16x32 B2)
    ('gemm', 'peaked', 'bf16'): (2.44e-03, 9.95e-03),     # bound F 9.76e-03, S 1.99e-02; device F 9.69e-04 (C128 16x32 B2), S 1.15e-02 (C640 16x16 B2)
    ('gemm', 'peaked', 'f16'): (2.97e-04, 1.97e-01),      # bound F 1.19e-03, S 3.94e-01; device F 3.61e-04 (C128 16x32 B2), S 1.34e-01 (C640 16x16 B2)
    ('gemm', 'peaked', 'f32'): 63.50,                     # bound C 254; device 42.1 (C64 16x32 B2)
    ('gemm', 'peaked', 'f32x3'): 279.12,                  # bound C 1116; device 268.5 (C128 24x24 B1)
    ('stream', 'flat', 'bf16'): (1.45e-04, 1.25e-01),     # bound F 5.80e-04, S 2.50e-01; device F 1.28e-04 (C128 24x24 B2), S 1.14e-01 (C896 24x24 B1)
    ('stream', 'flat', 'f16'): (2.19e-05, 3.17e-01),      # bound F 8.76e-05, S 4.00e-01; device F 1.83e-05 (C128 24x24 B2), S 2.82e-01 (C1024 24x24 B1)
    ('stream', 'large_logit', 'bf16'): (9.52e-04, 4.58e-03),# bound F 3.81e-03, S 9.16e-03; device F 3.57e-04 (C128 24x24 B2), S 3.20e-03 (C128 24x24 B2)
    ('stream', 'large_logit', 'f16'): (8.23e-04, 5.62e-02),# bound F 3.29e-03, S 1.12e-01; device F 8.47e-04 (C128 24x24 B2), S 3.33e-02 (C128 24x24 B2)
    ('stream', 'locator', 'bf16'): (2.54e-04, 4.83e-03),  # bound F 1.02e-03, S 9.66e-03; device F 2.54e-04 (C256 32x32 B1), S 4.62e-03 (C1024 24x24 B1)
    ('stream', 'locator', 'f16'): (1.18e-04, 4.55e-02),   # bound F 4.72e-04, S 9.10e-02; device F 8.68e-05 (C128 64x64 B1), S 2.67e-02 (C1024 24x24 B1)
    ('stream', 'peaked', 'bf16'): (9.39e-04, 7.74e-03),   # bound F 3.76e-03, S 1.55e-02; device F 9.40e-04 (C128 24x24 B2), S 5.15e-03 (C128 24x24 B2)
    ('stream', 'peaked', 'f16'): (3.06e-04, 9.69e-02),    # bound F 1.22e-03, S 1.94e-01; device F 2.46e-04 (C128 24x24 B2), S 5.69e-02 (C128 24x24 B2)
}


def bound16(group, fam, kind):
    """(F, S) of a 16-bit group: 4 x the emulation's F, twice its share (at least 1e-3, at most 0.4)"""
    f, s = NEED[(group, fam, kind)]
    return 4.0 * f, min(0.4, max(1e-3, 2.0 * s))


def bound32(group, fam, kind):
    return 4.0 * NEED[(group, fam, kind)]


def seed_of(C, H, W, fam):
    return 3000 + C + 7 * H + 3 * W + 100 * BASE.index(fam) if fam in BASE else 3900 + C


def perms(N):
    """the two token orders of the permutation tests: reversed, and a fixed random one"""
    return {"reversed": torch.arange(N - 1, -1, -1), "random": torch.randperm(N, generator=torch.Generator().manual_seed(N))}


def x3_roles(names, C, H, W, blocked):
    """f32x3: the product form (4 terms on gemmx3_*, 3 on the register-staged conv_*) of each GEMM of the block, by the map and channel counts in its profile name.
    Launches of one shape share a kernel unless their output layout differs -- only V's channel-major store, which the LDS-DMA GEMM does not take."""
    from test_gpu_conv_fwd_ref import _x3_form
    N = H * W
    one = [n for n in names if "1x1" in n.split("|")[0]]
    qb = 256 if N % 256 == 0 else 128 if N % 128 == 0 else 64
    smap = f"{H}x{W}" if not blocked else f"{qb // (8 if qb == 64 else 16)}x{8 if qb == 64 else 16}"
    v_gemm = N == 256 and C % 256 == 0
    want = {"qk": (f"{H}x{W}", C, 2 * C), "s": (smap, C, N), "pv": (smap, N, C), "proj": (f"{H}x{W}", C, C),
            "v": (f"{C // 16}x16", C, N) if v_gemm else (f"{H}x{W}", C, C)}
    out = {}
    for role, (mp, cin, cout) in want.items():
        forms = {_x3_form(n) for n in one if (n.split("|")[1] + " ").startswith(f"{mp} {cin}->{cout} ")}
        assert forms, (role, want[role], names)
        out[role] = forms.pop() if len(forms) == 1 else (3 if role == "v" and not v_gemm else 4)
    return out


def core_check(path, names, kind, C, H, W):
    """assert the core that ran, by its profile name"""
    attn = [n for n in names if n.startswith("attn_")]
    N = H * W
    if path in ("gemm3", "blocked"):
        assert not attn, names
        tails = [n.split("|")[1] for n in names if "1x1" in n.split("|")[0]]
        assert any(f" {C}->{N}" in t for t in tails) and any(f" {N}->{C}" in t for t in tails), names       # Q.K^T and P.V as GEMM launches
        if path == "blocked":
            qb = 256 if N % 256 == 0 else 128 if N % 128 == 0 else 64
            assert any(t.startswith(f"{qb // (8 if qb == 64 else 16)}x{8 if qb == 64 else 16} {C}->{N}") for t in tails), names
        return
    assert len(attn) == 1, names
    n = attn[0]
    sub = {"folded1": "attn_fused_n256tq_", "folded_ext": "attn_fused_n256t_", "fused": "attn_fused_n256_", "bdiag": "attn_fused_n64x4t_", "stream": "attn_stream_q64k64_"}[path]
    assert n.startswith(sub + kind + "|"), (sub, names)
    if path == "folded1":
        assert "qproj+" in n and "+proj" in n, n
    elif path in ("folded_ext", "bdiag"):
        assert "proj" not in n, n
    elif path == "fused":
        assert ("+proj" in n) == (C <= 512), n


_REFS = {}


def reference(form, C, H, W, B, fam, kind, x3=4):
    """(sd, x, ref, M), computed once per module and never changed"""
    key = (form, C, H, W, B, fam, kind, tuple(sorted(x3.items())) if isinstance(x3, dict) else x3)
    if key not in _REFS:
        sd, x = family(fam, C, B, H, W, seed_of(C, H, W, fam))
        _REFS[key] = (sd, x) + attn_block_ref(sd, "at_ref", x, kind, form, x3=x3)
    return _REFS[key]


def _run(f, env):
    from test_gpu_conv_fwd_ref import _run as run
    return run(f, env)


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_util


def _id(c, fam, kind):
    return f"{c[0]}-{kind}-{fam}-C{c[3]}-{c[4]}x{c[5]}-B{c[6]}"


PARAMS = [pytest.param(c, fam, kind, id=_id(c, fam, kind)) for c in CASES for fam in c[7] for kind in c[8]]


@pytest.mark.parametrize("case,fam,kind", PARAMS)
def test_attn_block(gu, case, fam, kind):
    path, form, group, C, H, W, B, _, _, env = case
    sd, x = family(fam, C, B, H, W, seed_of(C, H, W, fam))
    got, names = _run(lambda: gu.attn(sd, "at_ref", x, kind), env)
    core_check(path, names, kind, C, H, W)
    what = f"{path} {fam} C{C} {H}x{W} B{B}"
    assert bool(torch.isfinite(got).all()), what
    if kind in H16:
        _, _, ref, M = reference(form, C, H, W, B, fam, kind)
        F_, S = bound16(group, fam, kind)
        worst, f, s = check16(got, ref, M, kind, F_, S, what)
        print(f"MEASURE attn {group} {fam} {kind} {what} ulps={worst:.2f} F={f:.3e} share={s:.3e}")
    else:
        x3 = x3_roles(names, C, H, W, path == "blocked") if kind == "f32x3" else 4
        _, _, ref, M = reference(form, C, H, W, B, fam, kind, x3)
        c = check32(got, ref, M, bound32(group, fam, kind), what)
        print(f"MEASURE attn {group} {fam} {kind} {what} C={c:.2f} x3={x3}")


@pytest.mark.parametrize("kind", K16)
@pytest.mark.parametrize("order", ["reversed", "random"])
@pytest.mark.parametrize("case", PERM_CASES, ids=lambda c: c[0])
def test_token_permutation(gu, case, order, kind):
    """GroupNorm and attention commute with a permutation of the tokens: the permuted locator input, un-permuted again, meets the reference of the original within the
    same bounds -- every query's peak sits in another key block and lane, and in the streaming core the running maximum moves at other blocks"""
    path, form, group, C, H, W, B, env = case
    sd, x, ref, M = reference(form, C, H, W, B, "locator", kind)
    perm = perms(H * W)[order]
    got, names = _run(lambda: gu.attn(sd, "at_ref", permute_tokens(x, perm), kind), env)
    core_check(path, names, kind, C, H, W)
    got = permute_tokens(got, torch.argsort(perm))
    F_, S = bound16(group, "locator", kind)
    worst, f, s = check16(got, ref, M, kind, F_, S, f"{path} {order}")
    print(f"MEASURE attn {group} locator {kind} {path} {order} tokens ulps={worst:.2f} F={f:.3e} share={s:.3e}")
