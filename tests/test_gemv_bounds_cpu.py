"""CPU checks of tests/helpers/gemv_bounds.py: the case tables of tests/test_gemv_bounds_gpu.py reach every instance of the default GEMV
dispatch (csrc/lm_step.hip, rst_launch_gemv) and the combinations the kernels treat separately, and the bounds asserted there are
satisfiable (plain fp32 torch stays inside) and discriminating (three emulated defects do not)."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import gemv_bounds as GB

INSTANCES = ([f"gemv<{B},{r}>" for B in (1, 2, 3, 4) for r in (2, 4)] + [f"gemv<{B},2,f32>" for B in (1, 2, 3, 4)]
             + ["norm", "norm_gate", "ksplit"])
FAMILIES = ["gemv", "gemv_f32", "norm", "norm_gate", "ksplit"]


def _routed():
    """[(route facts, has residual, gate_out, B, K)] over both tables."""
    out = [(GB.route_bf16(c), c[4], c[6], c[0], c[2]) for c in GB.CASES_BF16]
    return out + [(GB.route_f32(c), c[6], False, c[0], c[1]) for c in GB.CASES_F32]


def test_tables_reach_every_instance():
    reached = {r["name"] for r, *_ in _routed()}
    assert len(INSTANCES) == 15
    lost = [n for n in INSTANCES if n not in reached]
    assert not lost, f"no case of CASES_BF16 + CASES_F32 reaches {lost} (reached: {sorted(reached)})"
    assert reached <= set(INSTANCES), f"route() names instances outside the list: {sorted(reached - set(INSTANCES))}"


def test_tables_hold_the_required_combinations():
    routed = _routed()

    def names(pred):
        return {r["name"] for r, res, gate, B, K in routed if pred(r, res, gate, B, K)}

    strided_res = names(lambda r, res, gate, B, K: r["strided"] and res)
    for what, ok in (("gemv<.,2>", lambda n: n.startswith("gemv<") and n.endswith(",2>")),
                     ("gemv<.,4>", lambda n: n.endswith(",4>")), ("gemv<.,2,f32>", lambda n: n.endswith("f32>")),
                     ("ksplit", lambda n: n == "ksplit")):
        assert any(ok(n) for n in strided_res), f"{what} lost its grid-strided case with a residual (have: {sorted(strided_res)})"
    strided = names(lambda r, *_: r["strided"])
    for n in ("norm", "norm_gate"):
        assert n in strided, f"{n} lost its grid-strided case"
    ragged = {r["family"] for r, *_ in routed if r["ragged"]}
    for fam in FAMILIES:
        assert fam in ragged, f"{fam} lost its case with a ragged last group"
    gated = {B for r, res, gate, B, K in routed if gate}
    for B in (1, 2, 3, 4):
        assert B in gated, f"gate_out lost its case at B = {B}"
    assert any(B * K == GB.LDS_FLOATS for r, res, gate, B, K in routed), "no case at the LDS limit B * K == 32768"
    # the budget of the cases a 2^24 threshold forces
    for c in GB.CASES_BF16:
        assert c[1] * c[2] <= 1.3 * 2 ** 24, c
    for c in GB.CASES_F32:
        assert c[1] * c[2] <= 1.3 * 2 ** 24, c


def test_route_thresholds():
    """The thresholds themselves, either side (lm_step.hip:536-541, 570)."""
    assert GB.route(1, 8176, 64)["name"] == "gemv<1,2>" and GB.route(1, 8177, 64)["name"] == "gemv<1,4>"
    assert GB.route(1, 4096, 4096, 1)["name"] == "norm" and GB.route(1, 4095, 4096, 1)["name"] == "gemv<1,2>"
    assert GB.route(2, 4096, 4096, 1)["name"] == "gemv<2,2>" and GB.route(1, 8192, 4104, 1)["name"] == "gemv<1,4>"
    assert GB.route(1, 8202, 2048, 1, True)["name"] == "norm_gate" and GB.route(1, 8202, 2048, 0, True)["name"] == "gemv<1,2>"
    assert GB.route(1, 8192, 2048)["name"] == "ksplit" and GB.route(1, 16384, 1024)["name"] == "gemv<1,4>"
    assert GB.route(1, 8192, 2048, 2)["name"] == "gemv<1,4>" and GB.route(2, 8192, 2048)["name"] == "gemv<2,4>"
    assert GB.route(4, 6144, 3072)["grid"] == 768 and GB.route(4, 6152, 3080)["grid"] == 512          # 48 KiB of stage, and above
    assert GB.route(1, 8203, 2056, 1) == dict(name="norm", family="norm", groups=1026, grid=513, strided=True, ragged=True, lds=8224)
    assert GB.route(3, 12, 8, 3, False, True, 1)["name"] == "gemv<3,2,f32>"
    assert GB.route(1, 8201, 2056)["groups"] == 1026 and GB.route(1, 8201, 2056)["grid"] == 1024


# ---- the bounds: satisfiable and discriminating -----------------------------------------------------------------------------------------
SMALL = 1 << 22      # cases of at most 4M weight elements: every family of operation, seconds of CPU time in all
SMALL_BF16 = [c for c in GB.CASES_BF16 if c[1] * c[2] <= SMALL]
SMALL_F32 = [c for c in GB.CASES_F32 if c[1] * c[2] <= SMALL]


def _fp32_bf16(case, o):
    """The operation of ops.gemv_bf16 in plain fp32 torch: P(x) in fp32, F.linear in fp32 against the bf16-valued weights."""
    B, N, K, mode, res, bias, gate = case
    x = o["x"]
    if mode == 1:
        P = x * (o["alpha"] * torch.rsqrt(GB.EPS_RMS + (x * x).mean(dim=1, keepdim=True)))
    elif mode == 2:
        P = F.silu(x[:, :K]) * x[:, K:]
    else:
        P = x
    h = F.linear(P, o["w"].float(), o["bias"])
    if gate:
        return F.silu(h[:, :N // 2]) * h[:, N // 2:]
    return o["res"] + h if res else h


def _ln_one_pass(x, gamma, beta, eps):
    m = x.mean(-1, keepdim=True)
    v = ((x * x).mean(-1, keepdim=True) - m * m).clamp_min(0)
    return (x - m) * torch.rsqrt(v + eps) * gamma + beta


def _fp32_f32(case, o, ln_fn=None):
    M, K, N, ln, bias, gelu, res, scale, _ = case
    a = o["x"]
    if ln:
        a = ln_fn(a, o["gamma"], o["beta"], GB.EPS_LN) if ln_fn else F.layer_norm(a, (K,), o["gamma"], o["beta"], GB.EPS_LN)
    y = F.linear(a, o["w"], o["bias"])
    if gelu:
        y = F.gelu(y)
    return o["res"] + o["scale"] * y if res else y


def _ratio(y, ref, bound):
    return ((y.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


def test_there_are_three_small_cases_per_family():
    plain = [c for c in SMALL_BF16 if c[3] == 0 and not c[6]]
    rms = [c for c in SMALL_BF16 if c[3] == 1 and not c[6]]
    silu = [c for c in SMALL_BF16 if c[3] == 2]
    gated = [c for c in SMALL_BF16 if c[6]]
    ln = [c for c in SMALL_F32 if c[3]]
    no_ln = [c for c in SMALL_F32 if not c[3]]
    for name, cs in (("plain", plain), ("RMSNorm", rms), ("SiLU gate", silu), ("gate_out", gated), ("LayerNorm", ln), ("fp32 plain", no_ln)):
        assert len(cs) >= 3, (name, cs)


@pytest.mark.parametrize("case", SMALL_BF16, ids=str)
def test_fp32_torch_is_within_the_bf16_bound(case):
    o = GB.operands_bf16(case)
    ref, bound = GB.reference_bf16(case, o)
    r = _ratio(_fp32_bf16(case, o), ref, bound)
    assert r <= 1, f"{case}: plain fp32 torch is at {r:.3g} of the bound"


@pytest.mark.parametrize("case", SMALL_F32, ids=str)
def test_fp32_torch_is_within_the_f32_bound(case):
    o = GB.operands_f32(case)
    ref, bound = GB.reference_f32(case, o)
    r = _ratio(_fp32_f32(case, o), ref, bound)
    assert r <= 1, f"{case}: plain fp32 torch is at {r:.3g} of the bound"


@pytest.mark.parametrize("case", [c for c in SMALL_F32 if c[3] and c[8]], ids=str)
def test_one_pass_variance_breaks_the_bound(case):
    """E[x^2] - E[x]^2 in fp32 on the row 1000 + randn (row 0 of the cases with planted rows): the variance of 1 is a difference of two
    numbers near 10^6, each good to 2^-24 of that."""
    o = GB.operands_f32(case)
    ref, bound = GB.reference_f32(case, o)
    y = _fp32_f32(case, o, _ln_one_pass)
    r = _ratio(y[:1], ref[:1], bound[:1])
    assert r > 1, f"{case}: the one-pass variance stays at {r:.3g} of the bound"


@pytest.mark.parametrize("case", [c for c in SMALL_BF16 if c[6] and c[5]], ids=str)
def test_the_u_bias_on_the_v_half_breaks_the_bound(case):
    """bias[q] in place of bias[half + q] (fp64 otherwise)."""
    o = GB.operands_bf16(case)
    ref, bound = GB.reference_bf16(case, o)
    half = case[1] // 2
    bad = o["bias"].clone()
    bad[half:] = bad[:half]
    y, _ = GB.reference_bf16(case, o, bias=bad)
    assert _ratio(y, ref, bound) > 1, case


@pytest.mark.parametrize("case", [c for c in SMALL_BF16 if not c[6]][:12] + SMALL_F32, ids=str)
def test_dropping_the_last_8_k_breaks_the_bound(case):
    """The last 8 k of every row left out of the sum (fp64 otherwise): a lost tail chunk."""
    f32 = len(case) == 9
    o = GB.operands_f32(case) if f32 else GB.operands_bf16(case)
    fn = GB.reference_f32 if f32 else GB.reference_bf16
    ref, bound = fn(case, o)
    w = o["w64"].clone()
    w[:, -8:] = 0
    y, _ = fn(case, o, w64=w)
    assert _ratio(y, ref, bound) > 1, case
