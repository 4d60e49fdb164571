"""CPU checks of the ViT forward's plan (csrc/vit_plan.h: resolve_vit; read back through vfm_debug_vit_plan): what a forward launches is
resolved once, from the model, the batch and the calling thread's policy, and the read-back reports it without touching a device.  The cases
are tests/vit_plan_cases.py -- written from the launch ladders as they stood before the plan."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import pytest

from . import vit_plan_cases as vpc

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


def vit_config(lib, s):
    return lib.VitConfig(s.dim, s.depth, s.heads, s.mlp, 14, 16, s.patch_w)


@pytest.mark.parametrize("case", vpc.CASES, ids=lambda c: c.id)
def test_the_read_back_equals_the_table(built, case):
    with built.using(built.Config(**dict(case.cfg))):
        plan = built.vit_plan(vit_config(built, case.shape), case.shape.B, case.W, case.cus)
    want = dict(zip(built.VIT_STAGES, case.stages))
    want.update(launches=case.launches, trace=case.trace)
    assert plan == want, "\n".join(f"{k}: {plan[k]}  (table: {want[k]})" for k in want if plan[k] != want[k])


def test_the_table_covers_the_rule_boundaries_the_issue_names():
    by_id = {c.id: c for c in vpc.CASES}
    fused = lambda c: c.stages[2].startswith("vit_qkv_attention_kernel")                  # noqa: E731
    for B, on in ((24, True), (42, True), (54, True), (84, True), (86, True), (23, False), (44, False), (48, False)):
        assert fused(by_id[f"default-B{B}"]) == on, B
    for B, on in ((156, True), (168, True), (252, True), (84, False), (144, False), (192, False)):
        assert (by_id[f"default-B{B}"].stages[5].startswith("vit_mlp_kernel")) == on, B
    for B, on in ((70, True), (93, True), (69, False), (94, False), (96, False)):
        two = by_id[f"two-kernels-B{B}"]
        assert two.stages[2].startswith("vit_gemm_astat2_kernel<QKV") == on and two.stages[5].startswith("vit_gemm_astat2_kernel<GELU") == on, B
        assert by_id[f"default-B{B}"].stages[5].startswith("vit_gemm_astat2_kernel<GELU") == on, B
    assert by_id["default-B6"].launches == 63 and by_id["default-B6"].shape.depth == 12
    assert {c.trace for c in vpc.CASES} == {None, "qkv", "proj", "fc1", "fc2"}
    assert {c.cus for c in vpc.CASES} > {vpc.CUS}
    for c in vpc.CASES:
        assert sum(k is not None and ",dbg>" in k for k in c.stages) == (c.trace in ("proj", "fc2")), c.id   # one traced launch at most


def test_the_named_keys_only(built):
    lib = built.load()
    cfg = built.Config()
    with pytest.raises(RuntimeError, match="unknown key 'vit_gemm'"):
        cfg.set("vit_gemm", (-5 << 32) | 1)
    assert not hasattr(cfg, "set_vit_gemm") and not hasattr(lib, "vfm_debug_set_vit_gemm")
    for value in (0x7FEDCBA987654300, 0x1_0000_0008, 0):     # every bit of the pointer: above 2^32, and back to none
        assert cfg.set("vit_trace_buffer", value).get("vit_trace_buffer") == value
    with built.using(cfg.set("vit_trace_buffer", 1 << 40)):
        assert built.policy("vit_trace_buffer") == 1 << 40
    assert built.policy("vit_trace_buffer") == 0
    for key in ("vit_xcd", "vit_lds_min_wg", "vit_lds_shape", "vit_att_lds_min", "vit_wpw", "vit_astat_min", "vit_astat_nw",
                "vit_preprocess_patch", "vit_astat_two", "vit_hot_a", "vit_wide_tile", "vit_trace_fused", "vit_cfg_narrow", "vit_cfg_wide"):
        assert cfg.set(key, 3).get(key) == 3, key


def test_the_read_back_refuses_what_the_forward_refuses_with_its_message(built):
    """... before any device call: the forward is given fake pointers"""
    lib = built.load()
    buf = C.create_string_buffer(1024)
    cases = [
        (built.VitConfig(384, 12, 5, 1536, 14, 16, 21), 6, b"dim must be heads*64"),
        (built.VitConfig(1088, 12, 17, 1536, 14, 16, 21), 6, b"dim must be heads*64"),
        (built.VitConfig(384, 12, 6, 1500, 14, 16, 21), 6, b"bad mlp_dim / depth"),
        (built.VitConfig(384, 0, 6, 1536, 14, 16, 21), 6, b"bad mlp_dim / depth"),
        (built.VitConfig(384, 65, 6, 1536, 14, 16, 21), 6, b"bad mlp_dim / depth"),
        (built.VitConfig(384, 12, 6, 1536, 16, 16, 21), 6, b"bad patch grid"),
        (built.VitConfig(384, 12, 6, 1536, 14, 0, 21), 6, b"bad patch grid"),
        (built.VitConfig(384, 12, 6, 1536, 14, 16, 21), 0, b"bad patch grid"),
        (built.VitConfig(384, 12, 6, 1536, 14, 16, 32), 6, b"at most 512 tokens per image supported (got 513)"),
        (built.VitConfig(384, 12, 6, 1536, 14, 16, 21), 5000, b"batch of 5000 images too large"),
    ]
    for cfg, B, text in cases:
        assert lib.vfm_debug_vit_plan(C.byref(cfg), B, 1600, 256, buf, len(buf)) != 0
        message = lib.vfm_last_error()
        assert text in message, message
        assert lib.vfm_vit_forward(C.byref(cfg), 1, 1, B, 1200, 1600, 1, 1, 1 << 40, None) != 0
        assert lib.vfm_last_error() == message
    ok = built.VitConfig(384, 12, 6, 1536, 14, 16, 21)
    assert lib.vfm_debug_vit_plan(C.byref(ok), 6, 1600, 256, buf, 16) != 0 and b"buffer" in lib.vfm_last_error()
    assert lib.vfm_debug_vit_plan(None, 6, 1600, 256, buf, len(buf)) != 0 and b"bad argument" in lib.vfm_last_error()
    assert lib.vfm_debug_vit_plan(C.byref(ok), 6, 1600, -1, buf, len(buf)) != 0
    assert lib.vfm_vit_forward(C.byref(ok), None, 1, 6, 1200, 1600, 1, 1, 1 << 40, None) != 0 and b"null pointer" in lib.vfm_last_error()
    assert lib.vfm_debug_vit_plan(C.byref(ok), 6, 1600, 256, buf, len(buf)) == 0 and buf.value.startswith(b"pre=vit_preprocess_patch_kernel@2112x256+0 ")
