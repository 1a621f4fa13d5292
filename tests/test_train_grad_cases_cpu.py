"""What makes the assertions of tests/test_hip_train_grad_exact.py mean something, checked from the operands and the float64
references of tests/train_grad_cases.py and the library's host-only route queries alone (CPU).

The routes: the GPU test claims to run all 14 weight-gradient instantiations of skoots_amd/csrc/train.hip; that holds only if
the table's cases reach them, which `route` -- wgrad_route of train.hip itself, through sk_train_conv_wgrad_route -- decides
here: every name and boundary asserted below pins the library, the names sk_train_conv_wgrad_route_name lists must be the
ones written out in the table, and the route's numbers are held against train_grad_cases.plan, an independent restatement;
together with the edges each route family is meant to meet (batch 2, an upsampled second source, several chunks, several channel tiles, ragged
channels, chunks left empty by the 16-rounding).  The operands: the GPU test demands bit equality with float64, a fair demand
only while every partial sum of the kernels, in whatever order they run, is an exact fp32 value -- operands exact in the
16-bit type, sums of absolute products below 2^24 units, results inside the exact range of the type that stores them.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import train_grad_cases as T

IDS = [T.case_id(c) for c in T.ALL]
TYPES = ("fp16", "bf16")
RUNS = T.runs()


def _routes(family):
    return [(c, e, zp) for c, e, zp in RUNS if T.family(T.route(c, e, zp)) == family]


def test_routes_equal_the_written_ones_and_cover_every_instantiation():
    """`route` over the table returns the name written next to every case, per entry point exactly the reachable set, and
    the reachable sets are the 4 + 8 + 2 instantiations the entry points can launch without an SK_TUNING switch."""
    for case in T.ALL:
        for entry in T.ENTRIES:
            if not T.accepts(case, entry):
                assert T.named(case, entry) is None
                continue
            for zp in ((False, True) if entry == "f16" else (False,)):
                assert T.route(case, entry, zp) == T.named(case, entry, zp), (T.case_id(case), entry, zp)
    for entry in T.ENTRIES:
        assert {T.route(c, e, zp) for c, e, zp in RUNS if e == entry} == T.REACHABLE[entry]
    assert T.REACHABLE["fp32"] == {"wgrad_stem<false>", "wgrad<9>", "wgrad<8>", "wgrad<1>"}
    assert T.REACHABLE["f16"] == {"wgrad16x", "wgrad16y"} | {f"wgrad16{t}<{n}>" for t in ("t", "") for n in (9, 8, 1)}
    assert T.REACHABLE["stem_f16"] == {"wgrad_stem16", "wgrad_stem<true>"}
    assert sum(len(v) for v in T.REACHABLE.values()) == 14
    for entry in T.ENTRIES:
        for twin in (False, True):
            names = T.library_names(entry, twin)
            assert len(names) == len(set(names)) and set(names) == T.REACHABLE[entry], (entry, twin, names)


def test_every_route_family_meets_its_edges():
    """Per family: batch >= 2; more than one chunk an item; where the family admits them (everything but the stem kernels) an
    upsampled second source (ksize 3 only: every family but the stem's has a ksize-3 member), more than one cout tile and
    more than one cin tile; on wgrad<*> and wgrad16<*> cout = 5 with a cin that is no multiple of 32, for every ksize; for
    wgrad16x more than one x segment, more than one y and more than one z footprint, a chunk count that is no multiple of
    the 8-chunk launch round (surplus workgroups that must write nothing), fewer rows than the plan's and MORE rows than
    the plan's (so that the x kernel's count sizes the workspace and its last row ends at the sentinel tail), the latter
    with batch 2 as well; for wgrad16y the same round and a chunk that gets no column."""
    families = {T.family(T.route(c, e, zp)) for c, e, zp in RUNS}
    assert families == {"wgrad_stem<false>", "wgrad_stem<true>", "wgrad_stem16", "wgrad", "wgrad16", "wgrad16t", "wgrad16y",
                        "wgrad16x"}
    for fam in sorted(families):
        cases = [c for c, _, _ in _routes(fam)]
        assert any(c[0] >= 2 for c in cases), fam
        if fam == "wgrad16x":
            assert any(T.plan(c)["nchunk_x"] > c[0] for c in cases)
        else:
            assert any(T.plan(c)["nchunk_b"] > 1 for c in cases), fam
        if not fam.startswith("wgrad_stem"):
            assert any(len(c[2]) == 2 and c[2][1][1] == 1 for c in cases), fam
            assert any(c[3] > 32 for c in cases) and any(T.cin_of(c) > 32 for c in cases), fam
    for fam in ("wgrad", "wgrad16"):
        for k in (3, 2, 1):
            assert any(c[3] == 5 and T.cin_of(c) % 32 and c[4] == k for c, _, _ in _routes(fam)), (fam, k)
    xs = [c for c, _, _ in _routes("wgrad16x")]
    assert any(T.plan(c)["nxs"] > 1 for c in xs) and any(c[1][1] > 16 for c in xs) and any(c[1][2] > 16 for c in xs)
    assert any(T.plan(c)["nchunk_x"] % 8 for c in xs)
    # the x kernel's partial rows can be fewer or more than the plan's; the workspace is sized by the larger count.  Where
    # they are more, the workspace ends with the x kernel's last row: only there does the sentinel tail behind it see a
    # surplus workgroup of the launch round (chunk count no multiple of 8) or a row too many
    assert any(0 < T.plan(c)["nchunk_x"] < T.plan(c)["nchunk"] for c in xs)
    over = [c for c in xs if T.plan(c)["nchunk_x"] > T.plan(c)["nchunk"]]
    assert any(T.plan(c)["nchunk_x"] % 8 for c in over) and any(c[0] >= 2 for c in over)
    ys = [c for c, _, _ in _routes("wgrad16y")]
    assert any(T.plan(c)["nchunk"] % 8 for c in ys) and any(T.y_columns(c)[2] for c in ys)


def test_empty_chunk_cases_have_empty_chunks():
    """After sk_train_conv_wgrad_f16 / sk_train_stem_wgrad_f16 round `chunk` to 16, the named cases have chunks that start at or
    past the volume's end -- on each voxel-chunked 16-bit route: wgrad16<9>, wgrad16t<9>, wgrad_stem16 -- while the unrounded
    plan (the fp32 entry point) has none.  The issue's two candidates, spelt out."""
    hit = set()
    for case in T.EMPTY_CHUNK_CASES:
        p = T.plan(case)
        assert p["empty"] and not T.plan(case, "fp32")["empty"]
        nvox = case[1][0] * case[1][1] * case[1][2]
        assert all((i % p["nchunk_b"]) * p["chunk"] >= nvox for i in p["empty"])
        hit |= {T.route(case, e, zp) for c, e, zp in RUNS if c == case and e != "fp32"}
    assert {"wgrad16<9>", "wgrad16t<9>", "wgrad_stem16"} <= hit
    p = T.plan((2, (49, 44, 10), T.S128, 128, 3))
    assert (p["nchunk_b"], p["chunk"], p["empty"]) == (42, 528, [41, 83]) and 41 * 528 == 21648 > 49 * 44 * 10 == 21560
    p = T.plan((8, (79, 69, 16), T.S1, 32, 3))
    assert (p["nchunk_b"], p["chunk"]) == (170, 528) and p["empty"] == [170 * b + cb for b in range(8) for cb in range(166, 170)]
    # every other case keeps chunk >= 512 = what the plan chose: no empty chunk
    assert all(not T.plan(c)["empty"] for c in T.ALL if c not in T.EMPTY_CHUNK_CASES)


@pytest.mark.parametrize("case", T.ALL, ids=IDS)
def test_plan_and_workspace_agree(case):
    """The chunks cover the volume, chunks that the rounding did not empty are not empty, and the workspace is the larger of
    the two row counts times a row of cout cin k^3 + cout floats"""
    B, (ox, oy, oz), _, cout, k = case
    nvox = ox * oy * oz
    for entry in T.ENTRIES:
        p = T.plan(case, entry)
        rounded = entry == "f16" or (entry == "stem_f16" and oz % 16 == 0)
        assert (p["nchunk"], p["nchunk_b"], p["nchunk_x"]) == tuple(T.plan(case)[key] for key in ("nchunk", "nchunk_b", "nchunk_x"))
        assert p["nchunk"] == B * p["nchunk_b"] and p["nchunk_b"] * p["chunk"] >= nvox
        assert p["chunk"] % (16 if rounded else 2) == 0 and p["chunk"] >= 512
        assert len(p["empty"]) == B * (p["nchunk_b"] - (nvox + p["chunk"] - 1) // p["chunk"])
        if p["nchunk_x"]:
            assert p["nchunk_x"] == B * (oy // 16) * (oz // 16) * p["nxs"] and (p["nxs"] - 1) * p["xseg"] < ox <= p["nxs"] * p["xseg"]
    p = T.plan(case)
    row = cout * T.cin_of(case) * k ** 3 + cout
    assert T.workspace_floats(case) == max(p["nchunk"], p["nchunk_x"]) * row


def _probes():
    """the table and shapes around the x-marching kernel's conditions"""
    return T.ALL + [(B, (ox, oy, oz), [(c, 0)], cout, 3) for B in (1, 2, 3) for ox in (1, 2, 7, 64) for oy in (15, 16, 48)
                    for oz in (16, 32, 64) for c, cout in ((32, 32), (64, 128), (31, 32))]


@pytest.mark.parametrize("twin", [False, True])
def test_exported_workspace_size_is_the_mirrors(twin):
    """sk_train_conv_wgrad_workspace_floats (a host function) against the restated plan, over the table and over shapes around
    the x-marching kernel's conditions: with one or two planes its row count exceeds or equals the plan's and sizes the
    workspace (asserted for some probes of batch 1 and of batch >= 2), with more planes the plan's does"""
    from skoots_amd import _ffi
    probes = _probes()
    for B in (1, 2):
        assert any(T.plan(c)["nchunk_x"] > T.plan(c)["nchunk"] for c in probes if c[0] >= B)
    assert any(0 < T.plan(c)["nchunk_x"] < T.plan(c)["nchunk"] for c in probes)
    fn = getattr(_ffi.lib, "sk_train_conv_wgrad_workspace_floats" + ("_bf16" if twin else ""))
    for case in probes:
        B, (ox, oy, oz), _, cout, k = case
        assert int(fn(B, ox, oy, oz, cout, T.cin_of(case), k)) == T.workspace_floats(case), T.case_id(case)


def test_library_plan_equals_the_mirror():
    """Over the table and the probes, through every entry point that takes the case, with and without a zero page: the
    integers sk_train_conv_wgrad_route reports are the mirror's -- the chunking after the entry's 16-rounding, the x-marching
    kernel's rows and segments, wgrad16y's columns a chunk, the workspace size -- its `nchunk` is the row count the chosen
    kernel writes (wgrad16x: its own), the grid is what that kernel's launch geometry makes of them, and the bf16 twin
    answers the same."""
    for case in _probes():
        B, (ox, oy, oz), _, cout, k = case
        tiles = ((cout + 31) // 32) * ((T.cin_of(case) + 31) // 32)
        for entry in T.ENTRIES:
            if not T.accepts(case, entry):
                continue
            for zp in ((False, True) if entry == "f16" else (False,)):
                r, p, what = T.library_route(case, entry, zp), T.plan(case, entry), (T.case_id(case), entry, zp)
                name = r.name.decode()
                rows = p["nchunk_x"] if name == "wgrad16x" else p["nchunk"]
                assert (r.nchunk, r.nchunk_b, r.chunk, r.ngroup) == (rows, p["nchunk_b"], p["chunk"], p["ngroup"]), what
                assert (r.nchunk_x, r.nxs, r.xseg) == (p["nchunk_x"], p["nxs"], p["xseg"]), what
                assert r.workspace_floats == T.workspace_floats(case), what
                assert r.ncol_chunk == (T.y_columns(case)[1] if name == "wgrad16y" else 0), what
                if name in ("wgrad16x", "wgrad16y"):                # whole launch rounds of eight chunks
                    assert r.grid == (rows + 7) // 8 * 8 * tiles * (3 if name == "wgrad16y" else 1), what
                elif name.startswith("wgrad_stem"):
                    assert r.grid == rows, what
                else:
                    assert r.grid == rows * tiles * p["ngroup"], what
                assert bytes(T.library_route(case, entry, zp, twin=True)) == bytes(r), what


def test_route_boundaries():
    """Probes of the f16 dispatch without data: z 15 / 16 / 17, y 3 / 4 / 15 / 16, with and without a zero page, cin 31 / 32"""
    def r(oy, oz, zp, c=32, cout=32, k=3):
        return T.route((1, (8, oy, oz), [(c, 0)], cout, k), "f16", zp)
    for oz in (15, 17):
        for oy in (3, 4, 15, 16):
            assert r(oy, oz, True) == "wgrad16t<9>" and r(oy, oz, False) == "wgrad16<9>"
    assert [r(oy, 16, True) for oy in (3, 4, 15, 16)] == ["wgrad16t<9>", "wgrad16y", "wgrad16t<9>", "wgrad16x"]
    assert [r(oy, 32, True) for oy in (8, 12, 32)] == ["wgrad16y", "wgrad16y", "wgrad16x"]
    assert all(r(oy, 16, False) == "wgrad16<9>" for oy in (3, 4, 15, 16))
    for oy in (4, 16):
        assert r(oy, 16, True, c=31) == "wgrad16<9>" and r(oy, 16, True, cout=5) == "wgrad16<9>"
    assert r(16, 16, True, k=1) == "wgrad16t<1>" and r(16, 16, True, k=2) == "wgrad16t<8>"
    assert r(16, 16, True, c=31, k=1) == "wgrad16<1>" and r(16, 16, False, k=2) == "wgrad16<8>"
    # two sources: both must be whole lines
    assert T.route((1, (8, 16, 16), [(32, 0), (64, 1)], 32, 3), "f16", True) == "wgrad16x"
    # the stem entry looks at z alone; the fp32 entry at the source
    for oz, name in ((15, "wgrad_stem<true>"), (16, "wgrad_stem16"), (17, "wgrad_stem<true>"), (32, "wgrad_stem16")):
        assert T.route((1, (8, 5, oz), T.S1, 32, 3), "stem_f16") == name
    assert T.route((1, (8, 5, 16), T.S1, 32, 3), "fp32") == "wgrad_stem<false>"
    assert T.route((1, (8, 5, 16), T.S1, 32, 1), "fp32") == "wgrad<1>"
    assert T.route((1, (8, 6, 16), [(1, 1)], 32, 3), "fp32") == "wgrad<9>"
    assert not T.accepts((1, (8, 5, 16), T.S32, 32, 3), "stem_f16")


def test_wgrad64_is_the_weight_gradient():
    """The 27-products reference against float64 autograd: the first case of the table for the stem, for every ksize and for
    an upsampled second source"""
    def first(pred):
        return next(c for c in T.ALL if pred(c))
    picked = [first(T.is_stem), first(lambda c: len(c[2]) == 2 and c[2][1][1])] + [first(lambda c, k=k: c[4] == k and not T.is_stem(c))
                                                                                 for k in (3, 2, 1)]
    assert len(set(map(T.case_id, picked))) == 5
    for case in picked:
        srcs, dy = T.integer_operands(case)
        k = case[4]
        w = torch.zeros((case[3], T.cin_of(case), k, k, k), dtype=torch.float64, requires_grad=True)
        b = torch.zeros(case[3], dtype=torch.float64, requires_grad=True)
        x = T.assemble(case, [t.double() for t in srcs])
        y = F.conv3d(x, w, b, padding=1) if k == 3 else F.conv3d(x, w, b, stride=k)
        y.backward(dy.double())
        dw, db = T.wgrad64(case, srcs, dy)
        assert torch.equal(dw, w.grad) and torch.equal(db, b.grad), T.case_id(case)


@pytest.mark.parametrize("case", T.ALL, ids=IDS)
def test_weight_gradient_operands_are_exact(case):
    """For either 16-bit type and either image kind: the operands are integers the type holds (the device dy included: dy
    2^SCALE_K); the sum of |x| |dy16| over ALL voxels, in units of the operands' grain, stays below 2^24 for every output
    channel, so every partial sum in every order is an exact fp32 value; the expected gradients are exact fp32 values below
    2^24 units."""
    for entry in T.ENTRIES:
        if not T.accepts(case, entry):
            continue
        srcs, dy, dw, db = T.expected(case, entry)
        fine = T.uses_fine_image(case, entry)
        unit = T.FINE_UNIT if fine else 1.0
        dy16 = dy.double() * 2.0 ** T.SCALE_K
        assert torch.equal(dy16, dy16.round())
        xmax = max(float(t.abs().max()) for t in srcs) / unit
        for t in srcs:
            assert torch.equal(t.double() / unit, (t.double() / unit).round())
        if not fine:                                               # a 16-bit operand (an fp32 image is not)
            for ty in TYPES:
                assert xmax <= T.EXACT_INT[ty] and float(dy16.abs().max()) <= T.EXACT_INT[ty]
        else:
            assert entry != "f16" and xmax < 2 ** 16               # value + remainder of the bf16 build: 8 + 8 bits
        assert xmax * float(dy16.abs().sum(dim=(0, 2, 3, 4)).max()) < T.LIMIT
        assert float(dw.abs().max()) / unit * 2.0 ** T.SCALE_K < T.LIMIT and float(db.abs().max()) * 2.0 ** T.SCALE_K < T.LIMIT
        assert torch.equal(dw.float().double(), dw) and torch.equal(db.float().double(), db)
        assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0


def test_data_gradient_operands_are_exact():
    """sk_train_pack_weight's cases: forward weights that either type holds; data gradients (stored in the 16-bit type, for
    transposed = 2 scaled by 2^SCALE_K in the parity tensor) inside the exact-integer range of the narrower type."""
    for Co, Ci, k in T.PACK_FORWARD:
        w = T.pack_forward_weight(Co, Ci, k)
        assert torch.equal(w.half().float(), w) and torch.equal(w.bfloat16().float(), w) and w.unique().numel() > 100
        assert Co % 32 == 0 and Ci % (32 if k == 3 else 16) == 0
    assert {(32, 3), (64, 3), (128, 3)} <= {(co, k) for co, _, k in T.PACK_FORWARD}
    assert {2, 1} <= {k for _, _, k in T.PACK_FORWARD}
    lim = min(T.EXACT_INT.values())
    for i, (B, osp, Co, Ci, k, ranges) in enumerate(T.DGRAD_CASES):
        dy, w, dx = T.dgrad_expected(i)
        assert dx.shape == (B, Ci) + tuple(osp) and 0 < float(dx.abs().max()) <= lim
        assert float(dy.abs().max()) == 1 and float(w.abs().max()) == 1
        assert (k == 1 or not torch.equal(w, w.flip(2, 3, 4))) and Co % 32 == 0   # an unflipped tap would show
        assert any(lo > 0 for lo, n in ranges) and all(n in (32, 64, 128) and lo + n <= Ci for lo, n in ranges)
    for k in (3, 1):                                                # the whole input, both halves, a range off 0 inside a half
        mine = [(Ci, lo, n) for _, _, _, Ci, kk, ranges in T.DGRAD_CASES if kk == k for lo, n in ranges]
        assert any(lo == 0 and n == Ci for Ci, lo, n in mine)
        assert any(lo == 0 and 2 * n == Ci for Ci, lo, n in mine) and any(lo == n and 2 * n == Ci for Ci, lo, n in mine)
        assert any(lo > 0 and lo + n < Ci or lo > n for Ci, lo, n in mine)
    assert {k for *_, k, _ in T.DGRAD_CASES} == {3, 1}
    for i, (B, csp, Co, Ci) in enumerate(T.DGRAD2_CASES):
        dy, w, dx = T.dgrad2_expected(i)
        assert dx.shape == (B, Ci) + tuple(2 * v for v in csp)
        assert 0 < float(dx.abs().max()) * 2.0 ** T.SCALE_K <= lim
        for ax in (2, 3, 4):                                        # no parity can stand in for another
            assert not torch.equal(w, w.flip(ax))
        assert any(v % 2 for v in csp)
