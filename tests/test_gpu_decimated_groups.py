"""GPU: the decimated group mix (zh_decimator_paint_groups, k_mix_groups_decimated in csrc/mix_groups.hip) against a numpy f32
add-by-add group sum followed, per group, by the oracle's zo_decimator_paint (or a plain add where the group's mode is a bypass):
bit for bit in the rows and in the Decimators' states, over three buffers with carried state, for group sizes on both sides of the
tile forms' boundary (P <= 32: many groups a tile; P > 32: chunks of 32 voices), with every kind of rate mixed within one launch,
a span that is unaligned to the 64-frame tiles at both ends, a strided source view and canaries around the destination."""
import ctypes as C

import numpy as np
import pytest

from tests import hostile_cases as hc

pytestmark = pytest.mark.gpu
SR = 48000.0
F, SPAN = 200, (3, 197)
BUFFERS = 3
# (fake_sample_rate, bypass): bypass; the hold at three rates; == and > the sample rate (add and reset); 0 and a negative rate (nothing
# painted); 1 Hz: no frame of a buffer samples, the carried dval plays; NaN and the infinities
MODES = [(6000.0, 1), (6000.0, 0), (1000.0, 0), (47999.0, 0), (48000.0, 0), (96000.0, 0), (0.0, 0), (-5.0, 0), (1.0, 0), (float("nan"), 0),
         (float("inf"), 0), (float("-inf"), 0)]


def _modes(G, P, b):
    """group g's mode in buffer b: all of MODES within a launch of many groups, and a group's mode changes between buffers"""
    return [MODES[(g + 5 * b + P) % len(MODES)] for g in range(G)]


def _reference(oracle, st, src, dst, P, modes, zero_first):
    """one call onto dst [G][>= F] (host), st: the groups' oracle Decimators"""
    L, (s, e) = oracle.lib(), SPAN
    for g, (fake, bypass) in enumerate(modes):
        mix = np.zeros(F, np.float32)                                  # +0 + voice 0 + voice 1 + ..., each sum rounded to f32
        for k in range(P):
            mix = mix + src[:, g * P + k]
        assert mix.dtype == np.float32
        row = np.ascontiguousarray(dst[g])
        if zero_first:
            row[s:e] = 0.0
        if bypass:
            L.zo_add_into(s, e, oracle.fptr(row), oracle.fptr(mix))
        else:
            L.zo_decimator_paint(C.byref(st[g]), s, e, oracle.fptr(row), SR, oracle.fptr(mix), fake)
        dst[g] = row


@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
@pytest.mark.parametrize("G", [1, 5, 65])
@pytest.mark.parametrize("P", [1, 3, 32, 33, 41])
def test_rows_and_states_equal_the_oracle_over_three_buffers(ctx, oracle, P, G, zero_first):
    import torch
    from zang_amd import modules as mod, zang
    V = G * P
    rng = np.random.default_rng([P, G, int(zero_first)])
    # zero_first: rows 16 bytes apart in multiples (the 16-byte loads where the form allows them); add: an odd stride (dword loads)
    stride = (V + 3) // 4 * 4 + 4 if zero_first else V + 1 + (V % 2)
    assert stride > V and (stride % 4 == 0) == zero_first
    backing = torch.full((F, stride), 7.0, dtype=torch.float32, device=ctx.device)
    image = backing[:, :V]
    dst_stride = F + 8
    dst_all = torch.full((G + 1, dst_stride), 0.5, dtype=torch.float32, device=ctx.device)
    dst = dst_all[:G]
    ref = np.full((G, dst_stride), 0.5, np.float32)
    m = mod.Decimator(G, ctx)
    st0 = m.state()
    assert st0["dval"].tolist() == [0.0] * G and st0["dcount"].tolist() == [1.0] * G
    st0["dval"], st0["dcount"] = 0.1 + 0.25 * np.arange(G), rng.random(G)  # a carried dval that shows where nothing samples
    st0["dcount"][::4] = 1.0                                               # init()'s
    m.set_state(st0)
    st = [oracle.Decimator(float(st0["dval"][g]), float(st0["dcount"][g])) for g in range(G)]
    loud = 0.0
    for b in range(BUFFERS):
        src = rng.uniform(-1.0, 1.0, (F, V)).astype(np.float32)
        image.copy_(torch.from_numpy(src))
        modes = _modes(G, P, b)
        dev_modes = m.group_modes([f for f, _ in modes], [y for _, y in modes])
        m.paint_groups(zang.Span(*SPAN), dst, image, P, SR, dev_modes, zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_mix_groups_decimated"], ctx.last_form()
        _reference(oracle, st, src, ref, P, modes, zero_first)
        got = dst_all.cpu().numpy()
        assert hc.same_f32(got[:G], ref), (f"buffer {b}", hc.first_difference(got[:G], ref), modes[:12])
        assert np.all(got[G] == 0.5), "the canary row beyond the last group"
        assert np.all(got[:, :SPAN[0]] == 0.5) and np.all(got[:, SPAN[1]:] == 0.5), "frames outside the span"
        have = m.state()
        want = np.array([(s.dval, s.dcount) for s in st], np.float32)
        assert hc.same_f32(np.stack([have["dval"], have["dcount"]], 1), want), (f"buffer {b}: state", have[:12], want[:12])
        loud = max(loud, float(np.abs(ref[:, SPAN[0]:SPAN[1]]).max()))
    assert torch.all(backing[:, V:] == 7.0)
    assert loud > 0.5                                                  # (one group: some buffer of its three paints something)
    m.close()


def test_bypass_on_every_group_is_the_plain_group_mix(ctx):
    """every group bypassed, zero-first: the bits of zh_mixdown_groups with ZH_PAINT_ZERO_FIRST (the yardstick that was there before);
    without zero-first: what dst held + that mix, ONE addition (addInto of the finished temps[2], example_polyphony.zig:162) -- not
    zh_mixdown_groups' `+=` of voice after voice onto dst.  The states stay."""
    import torch
    from zang_amd import modules as mod, zang
    P, G = 41, 7
    image = ctx.image(F, G * P)
    image.copy_(torch.rand((F, G * P), device=ctx.device) * 2 - 1)
    a, b, mix = (torch.full((G, F), 0.25, dtype=torch.float32, device=ctx.device) for _ in range(3))
    m = mod.Decimator(G, ctx)
    before = m.state().tobytes()
    bypass = m.group_modes([3000.0] * G, [1] * G)
    s, e = SPAN
    zang.mixdownGroups(zang.Span(s, e), mix, image, P, zero_first=True, ctx=ctx)
    m.paint_groups(zang.Span(s, e), a, image, P, SR, bypass, zero_first=True)
    m.paint_groups(zang.Span(s, e), b, image, P, SR, bypass)
    ctx.sync()
    assert torch.equal(a.view(torch.int32), mix.view(torch.int32)) and float(mix.abs().max()) > 1.0
    want = torch.full((G, F), 0.25, dtype=torch.float32, device=ctx.device)
    want[:, s:e] += mix[:, s:e]
    assert torch.equal(b.view(torch.int32), want.view(torch.int32))
    assert m.state().tobytes() == before
    m.close()


def test_return_codes(ctx):
    import torch
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_buf
    P, G = 3, 5
    image = ctx.image(F, G * P, fill=1.0)
    dst = torch.full((G, F), 0.5, dtype=torch.float32, device=ctx.device)
    m = mod.Decimator(G, ctx)
    modes = m.group_modes([6000.0] * G, [0] * G)
    sp, add, inv = zang.Span(*SPAN), abi.PAINT_ADD, abi.ZH_ERR_INVALID
    before = m.state().tobytes()
    assert m._paint_groups(sp, dst, image, P, SR, modes, abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_groups(sp, dst, image, 5, SR, modes, add) == inv                     # 3 groups of 5 for a Decimator of 5 voices
    assert m._paint_groups(sp, dst, image, 0, SR, modes, add) == inv
    assert m._paint_groups(sp, dst, image, 4, SR, modes, add) == inv                     # not a divisor
    assert m._paint_groups(zang.Span(5, 4), dst, image, P, SR, modes, add) == inv
    assert m._paint_groups(zang.Span(0, F + 1), dst, image, P, SR, modes, add) == inv
    lib, buf = ctx.lib, as_buf(image)
    assert lib.zh_decimator_paint_groups(m.handle, 3, 197, dst.data_ptr(), 100, buf, P, SR, modes.data_ptr(), add) == inv   # rows overlap
    assert lib.zh_decimator_paint_groups(m.handle, 3, 197, None, F, buf, P, SR, modes.data_ptr(), add) == inv
    assert lib.zh_decimator_paint_groups(m.handle, 3, 197, dst.data_ptr(), F, buf, P, SR, None, add) == inv
    assert lib.zh_decimator_paint_groups(None, 3, 197, dst.data_ptr(), F, buf, P, SR, modes.data_ptr(), add) == inv
    assert lib.zh_decimator_paint_groups(m.handle, 9, 9, dst.data_ptr(), F, buf, P, SR, modes.data_ptr(), abi.PAINT_ZERO_FIRST) == abi.ZH_OK   # nothing launched
    ctx.sync()
    assert m.state().tobytes() == before and torch.all(dst == 0.5)
    m.close()
