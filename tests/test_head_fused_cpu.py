"""Host side of hat_head_fused (no GPU): the descriptor mirror, the route switch, the shapes the wrapper accepts, and the plan
format, whose function table does not hold the entry (a plan records the head as the three launches it equals)."""
import ctypes as C

from super_resolution_amd import _lib, ops, plan
from super_resolution_amd.engine import Options


def test_descriptor_mirror_layout():
    d = _lib.HatHeadDesc
    assert C.sizeof(d) == 152 and d.B.offset == 96 and d.in_scale.offset == 128 and d.mean.offset == 132 and d.reserved0.offset == 148
    assert plan._pointer_fields(d) == list(range(0, 96, 8))           # twelve pointers lead the struct
    assert _lib.SIGNATURES["hat_head_fused"][1] == [C.POINTER(d), C.c_void_p]


def test_route_switch_and_plan_table():
    assert Options().no_head_fused is False
    assert Options.from_env({"HAT_NO_HEAD_FUSED": "1"}).no_head_fused and not Options.from_env({}).no_head_fused
    assert "hat_head_fused" not in plan.FN_IDS


def test_supported_shapes():
    pw = ops.PackedConv(None, None, 3, 3, 128, 9, 1, 144)
    assert ops.head_fused_supported(pw, 144, 16, ops.HAT_BF16) and ops.head_fused_supported(pw, 144, 0, ops.HAT_BF16)
    assert not ops.head_fused_supported(pw, 144, 16, ops.HAT_F32)      # the fp32 path keeps the three launches
    assert not ops.head_fused_supported(pw, 144, 24, ops.HAT_BF16)     # a wider ESC pool
    assert not ops.head_fused_supported(ops.PackedConv(None, None, 3, 3, 128, 12, 1, 180), 180, 16, ops.HAT_BF16)   # embed_dim 180
