"""CPU: the geometries of tests/paint_cases.py are what their table claims, the canary checker catches what it is there to catch,
and the oracle side of the in_place geometry is "zero the span, then paint".  On CPU tensors (torch aligns them to 64 bytes), from
data_ptr() and stride(0) alone: the GPU tests (tests/test_gpu_views.py) rely on these alignment classes to stand between a
misaligned view and a 16-byte access."""
import ctypes as C

import numpy as np
import pytest

from tests import paint_cases as pc

FRAMES, SPAN = 352, (13, 334)
VS = [256, 68]
ROLES = ("out", "in", "ctl")


def _geo(name, V):
    return pc.Geometry(name, V, frames=FRAMES, span=SPAN, delay_samples=100, device="cpu")


def _views(g):
    return {r: g.image(r) for r in ROLES}


def _row_ptrs(view):
    return [view.data_ptr() + 4 * r * view.stride(0) for r in range(view.shape[0])]


def _backing_of(g, view):
    for b in g.images:
        if b.t.untyped_storage().data_ptr() == view.untyped_storage().data_ptr():
            return b
    raise AssertionError("view without a backing")


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("name", list(pc.GEOMETRIES))
def test_every_view_has_the_shape_and_the_guards(name, V):
    g = _geo(name, V)
    for role, view in _views(g).items():
        assert tuple(view.shape) == (FRAMES, V) and view.stride(1) == 1 and view.stride(0) >= V
        b = _backing_of(g, view)
        assert b.t.data_ptr() % 64 == 0
        off_floats = (view.data_ptr() - b.t.data_ptr()) // 4
        row, col = divmod(off_floats, b.t.stride(0))
        assert row == pc.GUARD_ROWS and b.t.shape[0] == FRAMES + 2 * pc.GUARD_ROWS              # four guard rows above and below
        left, right = col, b.t.stride(0) - col - V
        assert (col, b.t.stride(0)) == g.layout(role)
        # off 5 with stride V + 8 leaves 3 floats right of a row (and 5 left of the next): the 8 between two rows are all guards
        assert left >= 4 and right >= 3 and left + right >= 8, (name, role, left, right)
        raw = b.t.view(__import__("torch").int32)
        outside = np.ones(tuple(b.t.shape), bool)
        if name != "shared_allocation":
            outside[row:row + FRAMES, col:col + V] = False
            assert (raw.numpy()[outside] == pc.CANARY).all()


@pytest.mark.parametrize("V", VS)
def test_alignment_classes_and_strides_are_what_the_table_claims(V):
    views = {n: _views(_geo(n, V)) for n in pc.GEOMETRIES}
    for role in ROLES:
        assert all(p % 16 == 0 for p in _row_ptrs(views["plain"][role])) and views["plain"][role].stride(0) == V + 8
        assert all(p % 16 == 4 for p in _row_ptrs(views["shifted"][role]))                       # base = 4 mod 16 in every row
        assert len({p % 16 for p in _row_ptrs(views["odd_stride"][role])}) > 1                   # rows change class
        assert _row_ptrs(views["odd_stride"][role])[0] % 16 == 0 and views["odd_stride"][role].stride(0) == V + 11
        assert all(p % 16 == 0 for p in _row_ptrs(views["mixed_aligned"][role]))                 # the vector forms stay on
        assert all(p % 16 == 0 for p in _row_ptrs(views["params_shifted"][role]))
    m = views["mixed_aligned"]
    assert [m[r].stride(0) for r in ROLES] == [V + 8, V + 24, V + 40]
    o = views["out_misaligned"]
    assert all(p % 16 == 4 for p in _row_ptrs(o["out"])) and all(p % 16 == 0 for r in ("in", "ctl") for p in _row_ptrs(o[r]))
    i = views["in_misaligned"]
    assert all(p % 16 == 0 for p in _row_ptrs(i["out"]))
    assert all(p % 16 == 12 for p in _row_ptrs(i["in"])) and i["in"].stride(0) == V + 12
    assert all(p % 16 == 8 for p in _row_ptrs(i["ctl"])) and i["ctl"].stride(0) == V + 16
    assert len({i[r].stride(0) for r in ROLES}) == 3
    p = views["in_place"]
    assert all(x % 16 == 4 for x in _row_ptrs(p["out"]))


@pytest.mark.parametrize("V", VS)
def test_shared_allocation_views_are_disjoint_elements_of_overlapping_ranges(V):
    g = _geo("shared_allocation", V)
    v = _views(g)
    assert len(g.images) == 1 and all(v[r].stride(0) == 3 * V + 24 for r in ROLES)
    elems = {}
    for r in ROLES:
        first = (v[r].data_ptr() - g.images[0].t.data_ptr()) // 4
        elems[r] = {first + f * v[r].stride(0) + c for f in (0, 1, FRAMES - 1) for c in range(V)}
        assert all(p % 16 == 0 for p in _row_ptrs(v[r]))
    assert not (elems["out"] & elems["in"]) and not (elems["out"] & elems["ctl"]) and not (elems["in"] & elems["ctl"])
    end = lambda t: t.data_ptr() + 4 * t.shape[0] * t.stride(0)                  # bufs_alias (csrc/common.hip.h): ptr + frames * stride
    for a in ROLES:
        for b in ROLES:
            assert v[a].data_ptr() < end(v[b])                                 # ... each way: the library calls them aliased
    again = g.image("out")                                                       # the one output view, back at the canary
    assert again.data_ptr() == v["out"].data_ptr() and len(g.images) == 1
    second = g.image("ctl")                                                      # a second control image opens a second tensor
    assert len(g.images) == 2 and second.stride(0) == 3 * V + 24


def _host_shared(g, V):
    """what Shared.target needs, without a device"""
    sh = pc.Shared.__new__(pc.Shared)
    sh.geo, sh.V, sh.F, sh.idx, sh.outs, sh.forms = g, V, g.frames, np.arange(3), [], {}
    sh.s, sh.e = g.span
    return sh


@pytest.mark.parametrize("V", VS)
def test_in_place_target_is_the_image_itself(V):
    import torch
    g = _geo("in_place", V)
    img = g.image("in", content=torch.arange(FRAMES * V, dtype=torch.float32).reshape(FRAMES, V))
    cols = np.ascontiguousarray(img[:, :3].numpy().T)
    sh = _host_shared(g, V)
    t = sh.target(img, cols)
    assert t.in_place and t.src.data_ptr() == t.o.data_ptr() and t.src.stride(0) == t.o.stride(0)      # the pointers are identical
    assert t.o.data_ptr() != img.data_ptr() and torch.equal(t.o, img)                                  # (a copy: the shared input stays)
    assert np.shares_memory(t.col(1), t.ref[1]) and not np.shares_memory(t.ref, cols) and np.array_equal(t.ref, cols)
    plain = _host_shared(_geo("plain", V), V)
    u = plain.target(img, cols)
    assert not u.in_place and u.src is img and u.o.data_ptr() != img.data_ptr() and not u.ref.any() and np.shares_memory(u.col(1), cols[1])


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("name", list(pc.GEOMETRIES))
def test_canary_checker_catches_guards_rows_inputs_and_params(name, V):
    import torch
    g = _geo(name, V)
    inp = g.image("in", content=torch.ones(FRAMES, V))
    ctl = g.image("ctl", content=torch.ones(FRAMES, V))
    out = g.image("out")
    pf = g.per_voice(np.arange(V, dtype=np.float32))
    pb = g.per_voice((np.arange(V) % 2).astype(np.uint8))
    assert pf.data_ptr() % 16 == 4 * g.pv_offset and pb.data_ptr() % 16 == g.pv_offset and pf.is_contiguous() and pb.is_contiguous()
    assert np.array_equal(pf.numpy(), np.arange(V, dtype=np.float32))
    g.check_canaries("untouched")
    s, e = SPAN
    out[s:e, :] = 0.25                                                          # only view x span changes: passes
    g.check_canaries("a paint")
    ob = _backing_of(g, out)
    off, _ = g.layout("out")

    def fails(t, index, value=0.5):
        old = t[index].clone()
        t[index] = value
        with pytest.raises(AssertionError, match="elements changed"):
            g.check_canaries("flipped")
        t[index] = old
        g.check_canaries("restored")

    fails(ob.t, (pc.GUARD_ROWS - 1, off))                                        # a guard row above
    fails(ob.t, (pc.GUARD_ROWS + FRAMES, off + V - 1))                           # ... below
    fails(ob.t, (pc.GUARD_ROWS + s, off - 1))                                    # a guard float left of a span row
    fails(ob.t, (pc.GUARD_ROWS + s, off + V))                                    # ... right of it (with stride == V: voice 0 of the next row)
    fails(out, (s - 1, 0))                                                       # a row of the view before the span
    fails(out, (e, V - 1))                                                       # ... after it
    fails(inp, (s, 3), 2.0)                                                      # an input element
    fails(ctl, (e - 1, V - 1), 2.0)                                              # a control element
    fails(pf, (5,), -1.0)                                                        # a per-voice value
    fails(pb, (V - 1,), 7)
    fails(g.arrays[0].t, (pc.PV_GUARD + g.pv_offset - 1,))                       # the guard element before a per-voice array
    fails(g.arrays[0].t, (pc.PV_GUARD + g.pv_offset + V,))                       # ... after it
    fails(g.arrays[1].t, (16 + g.pv_offset + V,), 1)


def _zero_then_paint_filter(oracle, s, e, start, ftype, cutoff, res, zf_seq):
    """written out by hand: zang.zero(span, out); filter.paint(span, .{out}, .{}, false, .{ .input = out, ... })"""
    L = oracle.lib()
    buf = start.copy()
    st = oracle.Filter(); L.zo_filter_init(C.byref(st))
    for zf in zf_seq:
        if zf:
            buf[s:e] = 0.0
        L.zo_filter_paint(C.byref(st), s, e, oracle.fptr(buf), oracle.fptr(buf), ftype, oracle.constant(cutoff), oracle.constant(res))
    return buf, (st.l, st.b)


def test_in_place_zero_first_reference_is_zero_then_paint(oracle):
    L = oracle.lib()
    s, e = SPAN
    rng = np.random.default_rng(3)
    start = rng.uniform(-1, 1, FRAMES).astype(np.float32)
    for zf_seq in ((True,), (False, True, False), (True, False)):
        for ftype in (1, 2, 4):
            ref = start.copy()
            st = pc.ref_filter(oracle, s, e, zf_seq, ref, None, ftype, 0.3, 0.4, True)
            want, wst = _zero_then_paint_filter(oracle, s, e, start, ftype, 0.3, 0.4, zf_seq)
            assert np.array_equal(ref.view(np.uint32), want.view(np.uint32)) and (st.l, st.b) == wst
            assert np.array_equal(ref[:s], start[:s]) and np.array_equal(ref[e:], start[e:])
            # ... which is NOT what painting the old contents onto a zeroed output gives (the fused form's mistake)
            other = start.copy(); other[s:e] = 0.0
            fl = oracle.Filter(); L.zo_filter_init(C.byref(fl))
            L.zo_filter_paint(C.byref(fl), s, e, oracle.fptr(other), oracle.fptr(start), ftype, oracle.constant(0.3), oracle.constant(0.4))
            if zf_seq == (True,):
                assert not np.array_equal(other, ref) and np.abs(other[s:e]).max() > 100 * np.abs(ref[s:e]).max()
        ref = start.copy()
        st = pc.ref_decimator(oracle, s, e, zf_seq, ref, None, 6000.0, True)
        want = start.copy()
        d = oracle.Decimator(); L.zo_decimator_init(C.byref(d))
        for zf in zf_seq:
            if zf:
                L.zo_zero(s, e, oracle.fptr(want))
            L.zo_decimator_paint(C.byref(d), s, e, oracle.fptr(want), pc.SR, oracle.fptr(want), 6000.0)
        assert np.array_equal(ref.view(np.uint32), want.view(np.uint32)) and (st.dval, st.dcount) == (d.dval, d.dcount)
        if zf_seq == (False, True, False):
            assert ref[s:e].any()                                               # the third paint adds the value the first one left held
    # not in place: the separate input column is read, the output starts from the zeros the test gives it
    col = rng.uniform(-1, 1, FRAMES).astype(np.float32)
    ref = np.zeros(FRAMES, np.float32)
    pc.ref_filter(oracle, s, e, (True, False), ref, col, 1, 0.3, 0.4, False)
    assert ref[s:e].any() and not ref[:s].any() and not ref[e:].any()


def test_walk_rows_are_the_rows_meant():
    """the `walks` forms of tests/test_gpu_views.py, derived from the library's table by name"""
    from tests.test_gpu_views import WALK_ROWS
    assert {"sine_ranges", "noise_ranges", "decimator_ranges", "script_ranges", "pulse_ctrl_ranges", "nice_pc_max", "nice_pc4_max", "nf_pc_max",
            "nf_ring_max", "filter_pc_max", "filter_pc16_max", "filter_pc_ctl_max", "pink_pipe_max", "echoes_pc_max", "delay_frames_max"} <= set(WALK_ROWS)
    assert not {"script_ranges_maxv", "script_pc_maxv", "filter_tp_max", "nice_wave_max", "basics_rows_min"} & set(WALK_ROWS)


class _StepsOnly:
    """what Shared.steps / pieces and noise_draws need of a Shared, without a device"""
    zf_seq = (True, False)
    steps, pieces = pc.Shared.steps, pc.Shared.pieces

    def __init__(self, g):
        self.geo = g
        self.s, self.e = g.span


def test_crafted_noise_draws_follow_the_span_length():
    """the positions of the crafted multi-draw samples at every length tests/test_gpu_span_lengths.py paints (noise_draws asserts
    its own conditions); at 1,024 frames they are the ones the dispatch tests always had"""
    for L in [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 136, 255, 256, 257, 321, 1024, 2047, 2048, 2049, 4103]:
        sh = _StepsOnly(pc.Geometry("plain", 132, frames=L + 11, span=(5, 5 + L), device="cpu"))
        a, b, c = pc.noise_draws(sh, "noise")
        d, e = pc.noise_draws(sh, "filter")
        assert min(a, b, c, d, e) >= 0
        if L >= 1:
            assert a < L and b < L and L <= c < 2 * L and d < L and L <= e < 2 * L, L
    sh = _StepsOnly(pc.Geometry("plain", 132, frames=1024, device="cpu"))
    assert pc.noise_draws(sh, "noise") == (77, 1001, 1539) and pc.noise_draws(sh, "filter") == (300, 1033)
    pieces = [(0, 127), (127, 255), (255, 256), (256, 320), (320, 383), (383, 1200)]
    sh = _StepsOnly(pc.Geometry("plain", 132, frames=1200, spans=pieces, device="cpu"))
    a, b, c = pc.noise_draws(sh, "noise")
    assert a < 127 and 127 + 64 <= b < 255 and 383 + 64 <= c < 1200


def test_steps_paint_one_span_twice_or_consecutive_spans_once():
    sh = _StepsOnly(pc.Geometry("plain", 8, frames=40, span=(3, 30), device="cpu"))
    assert sh.pieces() == [(3, 30, True), (3, 30, False)] and sh.pieces((False, True, False)) == [(3, 30, False), (3, 30, True), (3, 30, False)]
    sh = _StepsOnly(pc.Geometry("plain", 8, frames=40, spans=[(2, 9), (9, 10), (10, 33)], device="cpu"))
    assert sh.geo.span == (2, 33) and (sh.s, sh.e) == (2, 33)
    assert sh.pieces() == [(2, 9, True), (9, 10, False), (10, 33, False)] and (sh.s, sh.e) == (2, 33)
    assert sh.pieces((False, False)) == [(2, 9, False), (9, 10, False), (10, 33, False)]
    with pytest.raises(AssertionError):
        pc.Geometry("plain", 8, frames=40, spans=[(2, 9), (10, 33)], device="cpu")
