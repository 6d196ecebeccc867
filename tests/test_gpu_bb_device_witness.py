"""GPU tests of BabyBear witnesses created from DEVICE memory (msbb_witness_create_device, babybear.System.witness_from_device),
element for element: what msbb_witness_trace reads back is the caller's strided view, at every kernel form of csrc/ingest.hip
(ingest_vec_k, ingest_tiled_k, ingest_plain_k, instantiated for BbIngest at 1-, 2- and 4-byte elements). The counterpart of
tests/test_gpu_device_witness.py, whose BabyBear section goes through proof parity of one circuit of width 3.

Inputs are made with numpy from fixed seeds and moved with torch; narrow elements travel as signed tensors of the same bits.
Wherever a view does not reach, the memory under it holds 0xFF bytes: as a 4-byte element that is not canonical, so a read
outside the view is either copied (the comparison fails) or flagged (the call raises). Every comparison is exact.

Which form a case reaches - derived by READING launch() of csrc/ingest.hip, restated in dispatch() below and guarded by
test_case_table_reaches_every_form; no compiled code is looked at. For BabyBear the output axes are S = columns, F = rows,
ss = col_stride, fs = row_stride; PER = 16 / eb elements per 16-byte vector. Heights 1, 2, 64, 256; widths 1, 3, 16, 65, 130:

  layout       height    width      eb     form
  row          1         16         1 2 4  vec, S == 1 (one row is one run of 16 elements)
  row          1         1 3 65 130 1 2 4  plain, fs == 1 (w % PER != 0)
  row          2         1          1 2 4  plain, fs == 1
  row          64 256    1          1 2 4  vec, S == 1 (one column is one run)
  row          2         3 16       1 2 4  tiled, one ragged tile
  row          64        3 16       1 2 4  tiled, one tile, full along F
  row          256       3 16       1 2 4  tiled, 1 x 4 tiles (along S x along F)
  row          2 64      65 130     1 2 4  tiled, 2 x 1 and 3 x 1 tiles
  row          256       65 130     1 2 4  tiled, 2 x 4 and 3 x 4 tiles: full and ragged together on both axes
  col          any       any        1 2 4  the contiguous merge: vec, S == 1 where h * w % PER == 0 - every width at 64 and
                                           256 rows, width 16 at 1 and 2 rows, 2 x 130 at eb 4 - else plain, fs == 1
  colslice     1         any        1 2 4  plain, fs == 1 (merged, but the base lies 3 elements in: not aligned)
  colslice     2 64 256  1          1 2 4  plain, fs == 8, one column
  colslice     2 64 256  3 .. 130   1 2 4  tiled, as `row`
  rowstep      1         any        1 2 4  as `row`
  rowstep      2 64 256  1          1 2 4  plain, fs == 2, one column
  rowstep      2 64 256  3 .. 130   1 2 4  tiled, as `row`
  col_pitch16  64 256    3 .. 130   1 2 4  vec, S > 1: w aligned runs of h elements at a pitch of h + 16
  col_pitch16  64 256    1          1 2 4  vec, S == 1
  col_pitch16  1 2       any        1 2 4  plain, fs == 1 (h % PER != 0)
  col_pitch3   any       3 .. 130   1 2 4  plain, fs == 1: (h + 3) * eb is no multiple of 16 (or, at 1 and 2 rows, h % PER != 0)
  col_pitch3   64 256    1          1 2 4  vec, S == 1 (one column has no pitch)
  col_pitch3   1 2       1          1 2 4  plain, fs == 1
  col_rowstep  2 64 256  3 .. 130   1 2 4  plain, both strides non-unit: fs == 2, ss == 2 h
  col_rowstep  2 64 256  1          1 2 4  plain, fs == 2, one column
  col_rowstep  1         any        1 2 4  plain, fs == 1 (F == 1 takes the row stride away), ss == 2

The 2^19-row cases (width 16): (col_pitch16, 4) = 2^21 vectors in 16 runs, (row, 1) = 8192 tiles, (col_rowstep, 2) = 2^23
elements - each above one grid of its form (4096 workgroups of 256 threads, or 4096 tiles), as the restated
dispatch confirms: neither an element size nor the width had to be changed for a case to exceed one grid."""
import os

import numpy as np
import pytest
import torch

from __graft_entry__ import load_package
from test_gpu_device_witness import T, ff, layout, values as narrow_values

gpu = pytest.mark.gpu
pkg = load_package()
fe = pkg.frontend
bb = pkg.babybear
P = fe.BABYBEAR["P"]
assert P == 2013265921

WIDTHS = [1, 3, 16, 65, 130]
HEIGHTS = [1, 2, 64, 256]
LAYOUTS = ["row", "col", "colslice", "rowstep", "col_pitch16", "col_pitch3", "col_rowstep"]
EBS = [1, 2, 4]
MAX_BLOCKS, BLOCK = 4096, 256  # of csrc/ingest.hip


# ------------------------------------------------------------------ the dispatch of launch(), restated
def dispatch(h, w, row_stride, col_stride, eb, base_offset):
    """launch<In, BbIngest> of csrc/ingest.hip for an h x w view with strides in elements, eb-byte elements and a base
    `base_offset` bytes past a 16-byte boundary -> (form, S, F, detail): detail = vectors (vec), (tiles along S, tiles along F)
    (tiled) or (fs, ss, elements) (plain)"""
    S, F, ss, fs = w, h, col_stride, row_stride
    if F == 1:  # an axis of one element has no stride
        fs = 1
    if S == 1:
        ss = 0
    if fs == 1 and S > 1 and ss == F:  # contiguous: one long row
        F, S, ss = F * S, 1, 0
    per = 16 // eb
    if fs == 1 and F % per == 0 and base_offset % 16 == 0 and (ss * eb) % 16 == 0:
        return "vec", S, F, S * (F // per)
    if fs != 1 and ss == 1:
        return "tiled", S, F, ((S + 63) // 64, (F + 63) // 64)
    return "plain", S, F, (fs, ss, S * F)


def strides_of(kind, h, w):
    """(row_stride, col_stride, offset of the view's first element in elements) of layout `kind`, the allocation taken as
    16-byte aligned; an axis of one element is given the stride the formula gives (dispatch() ignores it, as launch() does)"""
    return {"row": (w, 1, 0), "col": (1, h, 0), "colslice": (w + 7, 1, 3), "rowstep": (2 * w, 1, 0),
            "col_pitch16": (1, h + 16, 0), "col_pitch3": (1, h + 3, 0), "col_rowstep": (2, 2 * h, 0)}[kind]


def form_of(kind, h, w, eb):
    rs, cs, off = strides_of(kind, h, w)
    return dispatch(h, w, rs, cs, eb, off * eb)


def bb_layout(t, kind):
    """the four layouts of the Goldilocks file and three column-major ones: the view and nothing else holds the values"""
    h, w = t.shape
    if kind in ("row", "col", "colslice", "rowstep"):
        return layout(t, kind)
    if kind in ("col_pitch16", "col_pitch3"):  # w runs of h elements, a pitch of h + 16 / h + 3 elements: strides (1, pitch)
        big = ff((w, h + (16 if kind == "col_pitch16" else 3)), t.dtype)
        view = big[:, :h].t()
    else:
        assert kind == "col_rowstep"  # column-major, every second row: strides (2, 2 h)
        big = ff((w, 2 * h), t.dtype)
        view = big[:, ::2].t()
    view.copy_(t)
    return view


def form_of_view(view):
    """dispatch() of what the library is handed for this tensor"""
    h, w = view.shape
    return dispatch(h, w, view.stride(0), view.stride(1), view.element_size(), view.data_ptr() % 16)


def bb_values(rng, h, w, eb):
    """eb 1, 2: the full range of the type, the maximum first and 0 last; eb 4: uniform below P with the edge values of the
    field and of its Montgomery form planted at seeded positions"""
    if eb < 4:
        return narrow_values(rng, h, w, eb)
    a = rng.integers(0, P, size=(h, w), dtype=np.uint64).astype(np.uint32)
    edges = np.array([0, 1, 2, P - 1, P - 2, 1 << 27, (1 << 27) + 1, 1 << 30], dtype=np.uint32)
    flat = a.reshape(-1)
    k = min(len(edges), flat.size)
    flat[rng.choice(flat.size, size=k, replace=False)] = edges[:k]
    return a


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context(0)
    bb.set_poseidon2(c, fe.poseidon2_constants())
    return c


def _no_jit(make):
    old = os.environ.get("MSAMD_NO_JIT")
    os.environ["MSAMD_NO_JIT"] = "1"  # nothing of these circuits is ever proved: no kernels to generate
    try:
        return make()
    finally:
        if old is None:
            del os.environ["MSAMD_NO_JIT"]
        else:
            os.environ["MSAMD_NO_JIT"] = old


@pytest.fixture(scope="module")
def wide(ctx):
    """(system, parameters, no claims): five circuits of main widths WIDTHS, one trivial constraint each, no lookups"""
    def circuit(w):
        def ev(b):
            m, mn = b.main()
            b.assert_zero(m[0] - mn[0])

        return fe.lookup_air(w, ev, [])

    with fe.field(fe.BABYBEAR):
        params = fe.test_params()
        system = _no_jit(lambda: bb.System.new(ctx, params, [circuit(w) for w in WIDTHS], fe.poseidon2_constants()))
        none = fe.pack_claims([])
    return system, params, none


def only(ci, view):
    out = [None] * len(WIDTHS)
    out[ci] = view
    return out


def assert_reads_back(w, ci, a):
    got = w.trace(ci)
    assert got.dtype == np.uint32 and got.shape == a.shape, "circuit %d: shape %r, expected %r" % (ci, got.shape, a.shape)
    want = a.astype(np.uint32)
    if not np.array_equal(got, want):
        r, c = np.argwhere(got != want)[0]
        raise AssertionError("circuit %d (width %d): %d elements differ, first at row %d, column %d: got %d, expected %d" % (
            ci, a.shape[1], int((got != want).sum()), r, c, got[r, c], want[r, c]))


# ------------------------------------------------------------------ 0. the guard of the case table (CPU)
def test_case_table_reaches_every_form():
    """the parametrization of test_exact_ingest reaches every kernel form, in each of its shapes, at each element size; the
    2^19-row cases exceed one grid of their form; the offender and commitment cases are of the form they are named after.
    (A guard against a later edit of the layouts dropping a form: it does not test the kernels.)"""
    assert dispatch(64, 3, 1, 64, 4, 0) == ("vec", 1, 192, 48)         # the existing suite's `col`: merged
    assert dispatch(64, 3, 3, 1, 4, 0) == ("tiled", 3, 64, (1, 1))     # and its `row`: one ragged tile
    assert dispatch(64, 3, 1, 64, 4, 4)[0] == "plain"                  # a base that is not aligned
    assert dispatch(64, 3, 1, 66, 4, 0)[0] == "plain"                  # a pitch that is not aligned: 264 bytes
    assert dispatch(64, 3, 1, 68, 4, 0) == ("vec", 3, 64, 48)
    assert dispatch(2, 3, 1, 68, 4, 0)[0] == "plain"                   # F % PER
    assert dispatch(1, 16, 99, 1, 1, 0) == ("vec", 1, 16, 1)           # F == 1: the row stride does not count
    assert dispatch(64, 1, 1, 99, 2, 0) == ("vec", 1, 64, 8)           # S == 1: nor the column stride
    for eb in EBS:
        seen = {}
        for kind in LAYOUTS:
            for h in HEIGHTS:
                for w in WIDTHS:
                    form, S, F, d = form_of(kind, h, w, eb)
                    if form == "vec":
                        key = "vec, S == 1" if S == 1 else "vec, S > 1"
                    elif form == "tiled":
                        key = "tiled, one tile" if d == (1, 1) else "tiled, several tiles along each axis" if min(d) > 1 else "tiled, other"
                        if min(d) > 1 and S % 64 and not F % 64:
                            seen.setdefault("tiled, ragged next to full along S", []).append((kind, h, w))
                    else:
                        fs, ss, _ = d
                        key = "plain, fs == 1" if fs == 1 else "plain, both strides non-unit" if ss > 1 else "plain, other"
                    seen.setdefault(key, []).append((kind, h, w))
        for key in ("vec, S == 1", "vec, S > 1", "tiled, one tile", "tiled, several tiles along each axis",
                    "tiled, ragged next to full along S", "plain, fs == 1", "plain, both strides non-unit"):
            assert seen.get(key), "eb %d: no case reaches '%s'" % (eb, key)
        # each new layout is there for one form
        assert all(form_of("col_pitch16", h, w, eb)[:2] == ("vec", w) for h in (64, 256) for w in WIDTHS[1:])
        assert all(form_of("col_pitch3", h, w, eb)[0] == "plain" and form_of("col_pitch3", h, w, eb)[3][0] == 1 for h in HEIGHTS for w in WIDTHS[1:])
        assert all(form_of("col_rowstep", h, w, eb)[0] == "plain" and form_of("col_rowstep", h, w, eb)[3][:2] == (2, 2 * h)
                   for h in HEIGHTS[1:] for w in WIDTHS[1:])
    for kind, eb in BIG_CASES:
        form, S, F, d = form_of(kind, 1 << 19, 16, eb)
        assert form == BIG_FORMS[kind]
        if form == "vec":
            assert S > 1 and d > MAX_BLOCKS * BLOCK
        elif form == "tiled":
            assert d[0] * d[1] > MAX_BLOCKS
        else:
            assert d[0] > 1 and d[1] > 1 and d[2] > MAX_BLOCKS * BLOCK
    for name, kind in FORM_CASES.items():
        for h, w in ((256, 130), (256, 65), (64, 65), (256, 16)):
            form, S, F, d = form_of(kind, h, w, 4)
            assert form == name.split("_")[0] and (name != "vec_merged" or S == 1) and (name != "vec_runs" or S == w), (name, h, w)
    form, S, F, d = form_of("row", 1 << 16, 16, 4)  # the producer-stream test
    assert form == "tiled"


# ------------------------------------------------------------------ 1. exact ingest
@gpu
@pytest.mark.parametrize("eb", EBS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_exact_ingest(wide, h, kind, eb):
    """all five circuits in one call; what the witness holds is the view, element for element; the 0xFF bytes around and between
    the view's elements are neither copied nor flagged (no exception)"""
    system, _, none = wide
    rng = np.random.default_rng(200000 + 100 * h + 10 * LAYOUTS.index(kind) + eb)
    arrs = [bb_values(rng, h, w, eb) for w in WIDTHS]
    views = [bb_layout(T(a), kind) for a in arrs]
    for v, wd in zip(views, WIDTHS):
        assert (v.data_ptr() - strides_of(kind, h, wd)[2] * eb) % 16 == 0, "the allocation is not 16-byte aligned"
        assert form_of_view(v) == form_of(kind, h, wd, eb), "the case table does not describe this tensor"
    w = system.witness_from_device(views, none)
    for ci, a in enumerate(arrs):
        assert_reads_back(w, ci, a)


BIG_CASES = [("col_pitch16", 4), ("row", 1), ("col_rowstep", 2)]
BIG_FORMS = {"col_pitch16": "vec", "row": "tiled", "col_rowstep": "plain"}


@gpu
@pytest.mark.parametrize("kind,eb", BIG_CASES)
def test_exact_ingest_more_work_than_one_grid(wide, kind, eb):
    """2^19 rows of width 16: 2^21 vectors in 16 runs, 8192 tiles, 2^23 elements - more than one grid of the largest size covers,
    so every form goes round its grid-stride loop (test_case_table_reaches_every_form checks the counts)"""
    system, _, none = wide
    h, ci = 1 << 19, WIDTHS.index(16)
    a = bb_values(np.random.default_rng(70 + eb), h, 16, eb)
    view = bb_layout(T(a), kind)
    assert view.data_ptr() % 16 == 0 and form_of_view(view) == form_of(kind, h, 16, eb)
    w = system.witness_from_device(only(ci, view), none)
    assert_reads_back(w, ci, a)
    assert w.trace(0).size == 0


@gpu
@pytest.mark.parametrize("kind", LAYOUTS)
def test_all_p_minus_one_is_accepted(wide, kind):
    system, _, none = wide
    ci = WIDTHS.index(65)
    a = np.full((64, 65), P - 1, dtype=np.uint32)
    w = system.witness_from_device(only(ci, bb_layout(T(a), kind)), none)
    assert_reads_back(w, ci, a)


# ------------------------------------------------------------------ 2. offenders
FORM_CASES = {"vec_merged": "col", "vec_runs": "col_pitch16", "tiled": "row", "plain": "col_pitch3"}


@gpu
@pytest.mark.parametrize("where", ["pair", "first", "last"])
@pytest.mark.parametrize("form", list(FORM_CASES))
@pytest.mark.parametrize("width", [130, 65])
def test_offender_is_named_in_every_form(wide, width, form, where):
    """pair: P at (200, 5) and 0xFFFFFFFF at (10, w - 3), in different tiles and workgroups. (10, w - 3) is the smaller r * w + c
    and must be named, although (200, 5) comes first in the kernels' own (column-major) output order - and, in the three forms
    whose source is column-major, first in the source's memory too. (A source of the tiled form has unit column stride: its
    memory order IS r * w + c, so there the output order alone is against the caller's.) Then one offender in the first and
    in the last element. After each refusal a good call on the same context reads back exactly."""
    system, _, none = wide
    h, ci, kind = 256, WIDTHS.index(width), FORM_CASES[form]
    good = bb_values(np.random.default_rng(300 + width), h, width, 4)
    a = good.copy()
    if where == "pair":
        a[200, 5], a[10, width - 3] = P, 0xFFFFFFFF
        r, c = 10, width - 3
        assert r * width + c < 200 * width + 5 and 5 * h + 200 < c * h + r
    elif where == "first":
        r, c = 0, 0
        a[r, c] = P
    else:
        r, c = h - 1, width - 1
        a[r, c] = 0xFFFFFFFF
    with pytest.raises(pkg.MstarkError, match=r"non-canonical trace value: circuit %d, row %d, column %d$" % (ci, r, c)):
        system.witness_from_device(only(ci, bb_layout(T(a), kind)), none)
    w = system.witness_from_device(only(ci, bb_layout(T(good), kind)), none)
    assert_reads_back(w, ci, good)


# ------------------------------------------------------------------ 3. independence from the read-back
@pytest.fixture(scope="module")
def uploaded(wide):
    """256 x 16 and 64 x 65 through System.witness, the upload path the suite pins to the oracle: arrays and the stage-1 cap"""
    system, params, none = wide
    rng = np.random.default_rng(400)
    arrs = {2: bb_values(rng, 256, 16, 4), 3: bb_values(rng, 64, 65, 4)}
    host = [arrs.get(ci, np.zeros((0, wd), dtype=np.uint32)) for ci, wd in enumerate(WIDTHS)]
    ldes = [a.shape[0] << params.log_blowup for a in host if a.shape[0]]
    cap = bb.commit_stage1(system.witness(host, none), params, ldes).cap
    assert len(cap) >= 8
    return arrs, ldes, cap


@gpu
@pytest.mark.parametrize("form", list(FORM_CASES))
def test_commitment_equals_that_of_the_uploaded_witness(wide, uploaded, form):
    """msbb_witness_trace and the ingest both turn the matrix, so a mistake made alike in both would cancel in the exact tests:
    the stage-1 commitment does not go through the read-back"""
    system, params, none = wide
    arrs, ldes, cap = uploaded
    views = [None] * len(WIDTHS)
    for ci, a in arrs.items():
        views[ci] = bb_layout(T(a), FORM_CASES[form])
    w = system.witness_from_device(views, none)
    got = bb.commit_stage1(w, params, ldes).cap
    assert got.shape == cap.shape and np.array_equal(got, cap)
    for ci, a in arrs.items():
        assert_reads_back(w, ci, a)


# ------------------------------------------------------------------ 4. stream ordering
@gpu
@pytest.mark.parametrize("how", ["explicit_handle", "current_stream"])
def test_producer_stream_is_waited_for(wide, how):
    """the trace is the end of a chain of 48 elementwise launches on a non-default stream, handed over without any synchronisation.
    (A pass does not prove the ordering - it guards against the argument being ignored.) The chain adds 1176 in all: the
    values stay below P."""
    system, _, none = wide
    h, steps, ci = 1 << 16, 48, WIDTHS.index(16)
    total = steps * (steps + 1) // 2
    base = np.random.default_rng(61).integers(0, P - total, size=(h, 16), dtype=np.uint64).astype(np.uint32)
    x0 = T(base)
    assert x0.dtype == torch.int32
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = x0
        for k in range(steps):
            x = x + (k + 1)
        if how == "explicit_handle":
            w = system.witness_from_device(only(ci, x), none, stream=side.cuda_stream)
        else:
            w = system.witness_from_device(only(ci, x), none)  # torch's current stream: `side`
    assert_reads_back(w, ci, base + np.uint32(total))
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------ 5. lifetime
@gpu
def test_sources_may_be_destroyed_after_the_call(ctx):
    with fe.field(fe.BABYBEAR):
        system = bb.System.new(ctx, fe.test_params(), fe.mul_air_inputs(), fe.poseidon2_constants())
        trace, none = fe.mul_air_trace(64), fe.pack_claims([])
    expect = system.prove_multiple_claims(system.witness([trace], none)).to_bytes()
    src = T(trace.astype(np.uint32))
    w = system.witness_from_device([src], none)
    src.zero_()
    del src
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    proof = system.prove_multiple_claims(w).to_bytes()
    assert proof == expect, "the proof differs from that of the uploaded witness"
    assert system.verify_multiple_claims(none, proof) == 0
