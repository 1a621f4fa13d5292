"""GPU tests of the Z-sharded labelling stage and of the kernels it rests on (sk_ccl_crop, sk_seam_pairs,
sk_compact_nonzero, sk_seam_union, sk_relabel_lut_offset, sk_relabel_lut, sk_first_seen), against scipy / numpy.

One process: the R ranks of a sharded run are R threads behind tests/inproc_comm.ThreadComm, all on the default stream of
the one device, so world sizes up to 8 and the production alignment (every rank's crop on the mask-driven ``ccl16_*`` path,
``z0`` = 32 or 48 inside a deeper window) run in a second or two.  Expected values come from tests/sharded_reference.py,
which tests/test_sharded_reference.py checks on the CPU.  Every comparison is an exact integer comparison."""
import numpy as np
import pytest
import scipy.ndimage
import torch

from oracle import pipeline as O
from tests import sharded_reference as R
from tests.inproc_comm import run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev():
    return torch.device(DEV)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(_dev())


# ----------------------------------------------------------------------------- the whole sharded stage
def _stage(mask, world, sync, sparse=None):
    """Run label_slab (or _label_slab_sync) on ``world`` rank threads; per rank (full volume, total, flag, call counts)."""
    from skoots_amd import parallel as P
    from skoots_amd.lib import flood_fill as F
    X, Y, Z = mask.shape
    slabs = P.slab_bounds(Z, world)
    windows = [P.window_of(s, Z, world) for s in slabs]
    dev = _dev()
    wins = [torch.from_numpy(np.array(mask[:, :, a:b], order="C")).to(dev) for a, b in windows]

    def body(comm):
        r = comm.rank
        if sync:
            full, total = F._label_slab_sync(wins[r], (X, Y, Z), slabs[r], windows[r], slabs, r, comm, sparse=sparse)
            flag = None
        else:
            full, total, flag = F.label_slab(wins[r], (X, Y, Z), slabs[r], windows[r], slabs, r, comm, sparse=sparse)
            flag = bool(flag.item())
        return full.cpu().numpy(), int(total), flag, dict(comm.calls)

    return run_ranks(world, body, timeout=120, device=dev)


def _assert_sync_path(mask, world, whole, counts, sparses=(None, True, False)):
    for sparse in sparses:
        res = _stage(mask, world, sync=True, sparse=sparse)
        for full, total, _, _ in res:
            assert total == sum(counts), sparse
            assert np.array_equal(full, res[0][0]), sparse
        assert R.partition_equal(res[0][0], whole), sparse


@pytest.mark.parametrize("name,world", R.CASE_IDS)
def test_label_slab_equals_scipy(name, world):
    mask = R.case_mask(name)
    whole, counts = R.case_reference(name, world)
    res = _stage(mask, world, sync=False)
    for full, total, flag, calls in res:
        assert calls["label_meta"] == 1 and calls["label_gather"] == 1, calls      # the sync-free path ran
    if name in R.FG_OVERFLOW:
        # a slab has more foreground voxels than the label gather carries: every rank must say so (the caller repeats the
        # stage on the host-synchronised path; nothing is promised about these labels)
        assert [flag for _, _, flag, _ in res] == [True] * world
    else:
        assert [flag for _, _, flag, _ in res] == [False] * world
        assert [total for _, total, _, _ in res] == [sum(counts)] * world
        for full, _, _, _ in res[1:]:
            assert np.array_equal(full, res[0][0])
        assert R.partition_equal(res[0][0], whole)
    _assert_sync_path(mask, world, whole, counts)


def test_seam_pair_overflow_is_flagged_and_the_sync_path_takes_over(monkeypatch):
    from skoots_amd.lib import flood_fill as F
    mask = R.case_mask("serpentine")
    whole, counts = R.case_reference("serpentine", 4)
    monkeypatch.setattr(F, "PAIR_CAP", 8)         # 256 bars cross every boundary
    res = _stage(mask, 4, sync=False)
    assert [flag for _, _, flag, _ in res] == [True] * 4
    assert all(calls["label_meta"] == 1 for _, _, _, calls in res)
    for sparse in (None, False):
        res = _stage(mask, 4, sync=True, sparse=sparse)
        assert all(calls["label_meta"] == 2 for _, _, _, calls in res)      # the second, exactly sized gather of the pairs
        assert [total for _, total, _, _ in res] == [sum(counts)] * 4
        assert R.partition_equal(res[0][0], whole)
    monkeypatch.setattr(F, "PAIR_CAP", 0)         # no sync-free path at all: label_slab itself answers, flag clear
    res = _stage(mask, 4, sync=False)
    assert [flag for _, _, flag, _ in res] == [False] * 4
    assert [total for _, total, _, _ in res] == [sum(counts)] * 4
    for full, _, _, _ in res:
        assert R.partition_equal(full, whole)


@pytest.mark.parametrize("shape", [(37, 29, 64), (16, 16, 256)])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_distributed_renumber_equals_oracle(shape, world):
    from skoots_amd import parallel as P
    rng = np.random.default_rng(shape[0] * 10 + world)
    X, Y, Z = shape
    max_label = 5000
    inst = rng.integers(0, max_label + 1, size=shape).astype(np.int32)
    inst[rng.random(shape) < 0.5] = 0
    slabs = P.slab_bounds(Z, world)
    for lo, _ in slabs[1:]:      # constant runs along z across every slab boundary
        for _ in range(40):
            x, y = int(rng.integers(0, X)), int(rng.integers(0, Y))
            a, b = max(0, lo - int(rng.integers(1, 6))), min(Z, lo + int(rng.integers(1, 6)))
            inst[x, y, a:b] = int(rng.integers(1, max_label + 1))
    ids = np.unique(inst)
    assert ids[-1] <= max_label and len(ids) < max_label        # gaps in the ids
    want, _ = O.renumber(inst)
    dev = _dev()

    def body(comm):
        lo, hi = slabs[comm.rank]
        mine = torch.from_numpy(np.ascontiguousarray(inst[:, :, lo:hi])).to(dev)
        k = P.distributed_renumber(mine, shape, (lo, hi), max_label, comm)
        return mine.cpu().numpy(), k

    res = run_ranks(world, body, timeout=60, device=dev)
    assert [k for _, k in res] == [int(want.max())] * world
    assert np.array_equal(np.concatenate([m for m, _ in res], axis=2), want)


# ----------------------------------------------------------------------------- sk_ccl_crop
def _ccl(vol_u8, box, state0):
    """sk_ccl_crop on a crop of a device volume; labels pre-filled with a sentinel.  Returns (labels, state)."""
    from skoots_amd import _ffi
    dev = _dev()
    Xv, Yv, Zv = vol_u8.shape
    x0, y0, z0, w, h, d = box
    labels = torch.full((Xv, Yv, Zv), -7, dtype=torch.int32, device=dev)
    ws_bytes = _ffi.lib.sk_ccl_workspace_bytes(w * h * d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    state = torch.tensor(state0, dtype=torch.int32, device=dev)
    _ffi.check(_ffi.lib.sk_ccl_crop(_ffi.ptr(vol_u8), _ffi.ptr(labels), Xv, Yv, Zv, x0, y0, z0, w, h, d, _ffi.ptr(ws), ws_bytes,
                                    _ffi.ptr(state), _ffi.stream_ptr(dev)))
    torch.cuda.synchronize()
    return labels.cpu().numpy(), state.cpu().tolist()


CCL_VOLUME = (24, 20, 160)
CCL_BOXES = [(0, 0, 16, 24, 20, 16), (0, 0, 16, 24, 20, 64), (0, 0, 48, 24, 20, 16), (0, 0, 48, 24, 20, 64),
             (3, 2, 48, 17, 15, 64), (5, 1, 16, 9, 18, 16)]


@pytest.mark.parametrize("fill", [0.02, 0.10, 0.35])
@pytest.mark.parametrize("box", CCL_BOXES)
def test_ccl_crop_mask_driven_path_away_from_the_origin(box, fill):
    """The crop of a slab inside its window: 16-aligned z0 > 0 and d inside a deeper, 16-aligned volume (the mask-driven
    ``ccl16_*`` kernels).  Foreground surrounds the crop, runs cross every 16-voxel chunk boundary (the crop's own first and
    last planes included).  Expected: scipy's numbering of the crop alone, first id ``state[0] + 2``; nothing written
    outside the crop; the same labels from the one-thread-per-voxel kernels (the crop embedded at an unaligned z0)."""
    X, Y, Z = CCL_VOLUME
    x0, y0, z0, w, h, d = box
    assert Z % 16 == 0 and z0 % 16 == 0 and d % 16 == 0 and 0 < z0 and z0 + d < Z
    rng = np.random.default_rng(int(fill * 100) * 1000 + sum(box))
    m = (rng.random(CCL_VOLUME) < fill).astype(np.uint8)
    for zb in range(16, Z, 16):
        m[:, :, zb - 1:zb + 1] |= (rng.random((X, Y, 1)) < 0.3).astype(np.uint8)
    crop = np.ascontiguousarray(m[x0:x0 + w, y0:y0 + h, z0:z0 + d])
    ref, k = scipy.ndimage.label(crop)
    assert k > 1
    dev = _dev()
    vol = torch.from_numpy(m).to(dev)
    wide = np.zeros((w, h, d + 16), dtype=np.uint8)      # z0 = 8: rows not 16-byte aligned -> generic kernels
    wide[:, :, 8:8 + d] = crop
    wide[:, :, 7] = 1                                      # foreground touching the crop from outside must not link
    wide_d = torch.from_numpy(wide).to(dev)
    for s0 in (-1, 1):
        want = np.where(ref > 0, ref + s0 + 1, 0).astype(np.int32)
        got, st = _ccl(vol, box, [s0, 0, 5, 0])
        inside = got[x0:x0 + w, y0:y0 + h, z0:z0 + d]
        assert np.array_equal(inside, want), s0
        outside = got.copy()
        outside[x0:x0 + w, y0:y0 + h, z0:z0 + d] = -7
        assert (outside == -7).all(), s0
        # state: [last id handed out, components of this crop, running total, id offset of this crop]
        assert st == [s0 + 1 + k, k, 5 + k, s0 + 1], (s0, st)
        slow, st_slow = _ccl(wide_d, (0, 0, 8, w, h, d), [s0, 0, 5, 0])
        assert np.array_equal(slow[:, :, 8:8 + d], want) and st_slow == st, s0


# ----------------------------------------------------------------------------- sk_seam_pairs
SEAM_SHAPE = (9, 70, 5)     # planes of 350, 45 and 630 positions: none a multiple of the 256-thread block


@pytest.fixture(scope="module")
def seam_labels():
    rng = np.random.default_rng(7)
    lab = rng.integers(0, 4, size=SEAM_SHAPE).astype(np.int32)      # few ids: runs along every axis, a quarter zeros
    lab[2:5, 10:30, :] = 9                                            # and one solid block
    lab.setflags(write=False)
    return lab, _i32(lab)


def _seam(lab_d, axis, v, capacity, slots):
    from skoots_amd import _ffi
    dev = _dev()
    X, Y, Z = SEAM_SHAPE
    pairs = torch.full((slots, 2), -1, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    _ffi.check(_ffi.lib.sk_seam_pairs(_ffi.ptr(lab_d), X, Y, Z, axis, v, _ffi.ptr(pairs), _ffi.ptr(count), capacity,
                                      _ffi.stream_ptr(dev)))
    torch.cuda.synchronize()
    return pairs.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_seam_pairs_every_axis(seam_labels, axis, where):
    lab, lab_d = seam_labels
    dim = SEAM_SHAPE[axis]
    v = {"first": 1, "middle": dim // 2, "last": dim - 1}[where]
    ref = R.seam_pair_set(lab, axis, v)
    adjacent = R.seam_adjacent(lab, axis, v)
    assert 3 < len(ref) <= adjacent
    slots = lab.size // dim + 8
    pairs, count = _seam(lab_d, axis, v, slots - 8, slots)
    print(f"axis {axis} v {v}: count {count}, distinct pairs {len(ref)}, adjacent positions {adjacent}, "
          f"runs {R.seam_runs(lab, axis, v)}")
    assert len(ref) <= count <= adjacent
    assert set(map(tuple, pairs[:count].tolist())) == ref
    assert (pairs[count:] == -1).all()
    # past capacity: the count goes on, the buffer is written up to the capacity only
    few, count3 = _seam(lab_d, axis, v, 3, slots)
    assert count3 == count
    assert all(tuple(p) in ref for p in few[:3].tolist())
    assert (few[3:] == -1).all()


# ----------------------------------------------------------------------------- sk_compact_nonzero
def _compact(lab_d, capacity, slots):
    from skoots_amd import _ffi
    dev = _dev()
    pos = torch.full((slots,), -1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    _ffi.check(_ffi.lib.sk_compact_nonzero(_ffi.ptr(lab_d), lab_d.numel(), _ffi.ptr(pos), _ffi.ptr(cnt), capacity,
                                           _ffi.stream_ptr(dev)))
    torch.cuda.synchronize()
    return pos.cpu().numpy(), int(cnt.item())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70001])
@pytest.mark.parametrize("density", [0.0, 0.01, 1.0])
def test_compact_nonzero(n, density):
    rng = np.random.default_rng(n + int(density * 100))
    lab = np.where(rng.random(n) < density, rng.integers(1, 1 << 30, size=n), 0).astype(np.int32)
    if density == 0.01:
        lab[n - 1] = 3          # the last element, in a wave that is not full
    want = np.flatnonzero(lab)
    lab_d = _i32(lab)
    pos, count = _compact(lab_d, n, n + 8)
    assert count == len(want)
    assert np.array_equal(np.sort(pos[:count]), want)
    assert (pos[count:] == -1).all()
    if count >= 2:      # past capacity: the count is the full number, `capacity` distinct non-zero positions are written
        cap = count // 2
        pos, count2 = _compact(lab_d, cap, n + 8)
        assert count2 == count
        assert len(np.unique(pos[:cap])) == cap and np.isin(pos[:cap], want).all()
        assert (pos[cap:] == -1).all()


# ----------------------------------------------------------------------------- sk_seam_union
def _union_case(n_ranks, clip, rng):
    """Hand-built metadata rows of ``n_ranks`` ranks.  Row r holds pairs (id of rank r + 1, id of rank r) in rank-local
    ids (the last row -- the only one when there is one rank -- pairs ids of its own rank: both columns take the same
    offset there).  Returns (meta, offsets, capacity, lut_size, the global pairs the kernel may use)."""
    counts = [6000 + 400 * r for r in range(n_ranks)]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    fresh = [list(rng.permutation(np.arange(1, c + 1))) for c in counts]      # unused local ids of every rank
    dead = 2 if n_ranks >= 5 else None          # a rank in the middle without any pair: nothing joins ranks 2 and 3
    rows = [[] for _ in range(n_ranks)]

    def node(rank):
        return (rank, int(fresh[rank].pop()))

    def link(a, b):
        (ra, ia), (rb, ib) = a, b
        if n_ranks == 1 or ra == rb:
            assert ra == rb == n_ranks - 1
            rows[ra].append((ia, ib))
        else:
            assert abs(ra - rb) == 1
            (rl, il), (ru, iu) = sorted([a, b])
            assert rl != dead
            rows[rl].append((iu, il))

    def walk(n, lo, hi):
        """n nodes, consecutive ones on neighbouring ranks of lo..hi (one rank: all on it)."""
        r = int(rng.integers(lo, hi + 1))
        out = [node(r)]
        for _ in range(n - 1):
            if hi > lo:
                r = r + 1 if r == lo else (r - 1 if r == hi else r + int(rng.choice([-1, 1])))
            out.append(node(r))
        return out

    if n_ranks == 1:
        spans = [(0, 0)]
    elif dead is None:
        spans = [(0, n_ranks - 1)]
    else:
        spans = [(0, dead), (dead + 1, n_ranks - 1)]
    lo, hi = spans[0]
    path = walk(4000, lo, hi)                              # one long path laid across the ranks
    for a, b in zip(path, path[1:]):
        link(a, b)
    lo, hi = spans[-1]
    centre = node(lo if hi == lo else lo + 1 if hi - lo >= 2 else lo)
    for _ in range(300):                                    # a star
        leaf_rank = centre[0] if hi == lo else (centre[0] + int(rng.choice([-1, 1])) if lo < centre[0] < hi
                                                else (centre[0] + 1 if centre[0] == lo else centre[0] - 1))
        link(node(leaf_rank), centre)
    q1, q2 = walk(200, lo, hi), walk(200, lo, hi)          # two components that touch at ONE edge
    for q in (q1, q2):
        for a, b in zip(q, q[1:]):
            link(a, b)
    link(*next((a, b) for a in q1[100:] for b in q2[50:] if hi == lo or abs(a[0] - b[0]) == 1))
    for _ in range(40):                                     # small separate components
        a = node(lo)
        link(a, node(lo + 1 if hi > lo else lo))
    for row in rows:                                        # duplicated pairs, then shuffled order
        if row:
            row += [row[int(i)] for i in rng.integers(0, len(row), size=150)]
            order = rng.permutation(len(row))
            row[:] = [row[int(i)] for i in order]
    lut_size = int(offsets[-1]) + 1 + 500
    # pairs that must be ignored: a global id of 0, a negative one, one past the table (first row: column 1 has offset 0)
    junk = [(7, 0), (7, -3), (int(lut_size), 9), (5, int(lut_size) + 11)]
    if n_ranks == 1:
        junk = [(0, 7), (7, -3), (int(lut_size), 9), (5, int(lut_size) + 11)]
    for j in junk:
        rows[0].insert(int(rng.integers(0, len(rows[0]) + 1)), j)
    longest = max(len(row) for row in rows)
    cap = longest - 120 if clip else longest + 10
    stride = 4 + 2 * cap
    meta = np.zeros((n_ranks, stride), dtype=np.int32)
    used = []
    for r, row in enumerate(rows):
        meta[r, 0], meta[r, 1] = counts[r], len(row)        # row[1] may exceed the capacity: only `cap` pairs exist
        meta[r, 2], meta[r, 3] = 12345 + r, 1                # the foreground count words, no business of the union
        kept = row[:cap]
        if kept:
            meta[r, 4:4 + 2 * len(kept)] = np.array(kept, dtype=np.int32).reshape(-1)
        o0, o1 = int(offsets[min(r + 1, n_ranks - 1)]), int(offsets[r])
        for a, b in kept:
            ga, gb = a + o0, b + o1
            if 0 < ga < lut_size and 0 < gb < lut_size:
                used.append((ga, gb))
    if clip:
        assert any(len(row) > cap for row in rows)
    if dead is not None:
        assert len(rows[dead]) == 0 and len(rows[dead + 1]) > 0 and len(rows[dead - 1]) > 0
    return meta, offsets, cap, lut_size, used


@pytest.mark.parametrize("n_ranks", [1, 2, 5, 8])
@pytest.mark.parametrize("clip", [False, True], ids=["fits", "clipped"])
def test_seam_union_gives_the_smallest_id_of_every_component(n_ranks, clip):
    """lut[id] == smallest id of id's component for every id of a used pair, the identity everywhere else (the contract
    in the kernel's comment).  The 4000-id path in shuffled order only closes through chains of other unions, and the
    kernel's link pass and point-at-root pass are separated by a workgroup barrier alone."""
    from skoots_amd import _ffi
    rng = np.random.default_rng(100 + n_ranks * 2 + clip)
    meta, offsets, cap, lut_size, used = _union_case(n_ranks, clip, rng)
    want = R.min_of_component(lut_size, used)
    if not clip:
        sizes = np.bincount(want)
        assert sizes.max() >= 4000 and (sizes == 301).any() and (sizes == 400).any() and (sizes == 2).sum() >= 40
    dev = _dev()
    meta_d = torch.from_numpy(meta).to(dev)
    off_d = torch.from_numpy(offsets).to(dev)
    lut = torch.arange(lut_size + 16, dtype=torch.int32, device=dev)     # 16 entries past the table: never touched
    _ffi.check(_ffi.lib.sk_seam_union(_ffi.ptr(meta_d), n_ranks, meta.shape[1], cap, _ffi.ptr(off_d), _ffi.ptr(lut), lut_size,
                                      _ffi.stream_ptr(dev)))
    torch.cuda.synchronize()
    got = lut.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[lut_size:], np.arange(lut_size, lut_size + 16))
    bad = np.flatnonzero(got[:lut_size] != want)
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])


# ----------------------------------------------------------------------------- sk_relabel_lut_offset, sk_relabel_lut
@pytest.mark.parametrize("n", [1, 257, 100003])
def test_relabel_lut_and_relabel_lut_offset(n):
    from skoots_amd import _ffi
    dev = _dev()
    rng = np.random.default_rng(n)
    lut_size, offset = 700, 250
    lab = rng.integers(0, 1000, size=n).astype(np.int32)
    lab[rng.random(n) < 0.3] = 0
    if n == 1:
        lab[0] = 600        # + offset: past the table
    lut = rng.integers(1, 1 << 30, size=lut_size).astype(np.int32)
    lut[::7] = np.arange(lut_size, dtype=np.int32)[::7]      # some identities
    lut_d = _i32(lut)
    st = _ffi.stream_ptr(dev)

    g = lab.astype(np.int64) + offset
    want = np.where(lab > 0, np.where(g < lut_size, lut[np.minimum(g, lut_size - 1)], g), lab).astype(np.int32)
    assert n == 1 or ((lab > 0) & (g >= lut_size)).any() and ((lab > 0) & (g < lut_size)).any() and (lab == 0).any()
    got = _i32(lab)
    off_d = torch.tensor([offset], dtype=torch.int64, device=dev)
    _ffi.check(_ffi.lib.sk_relabel_lut_offset(_ffi.ptr(got), n, _ffi.ptr(lut_d), lut_size, _ffi.ptr(off_d), st))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)

    want = np.where((lab > 0) & (lab < lut_size), lut[np.minimum(lab, lut_size - 1)], lab).astype(np.int32)
    got = _i32(lab)
    _ffi.check(_ffi.lib.sk_relabel_lut(_ffi.ptr(got), n, _ffi.ptr(lut_d), lut_size, st))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------- sk_first_seen (slab form)
def test_first_seen_slab_gives_global_first_appearance():
    from skoots_amd import _ffi
    dev = _dev()
    rng = np.random.default_rng(5)
    X, Y, zl, z_off, Zg, max_label = 13, 11, 24, 40, 100, 300
    lab = np.repeat(rng.integers(0, 401, size=(X, Y, zl // 3)), 3, axis=2).astype(np.int32)     # runs along z
    lab[rng.random(lab.shape) < 0.2] = 0
    rows = lab.reshape(-1, zl)      # a row that starts with the label the row before it ends with does NOT continue its run
    rows[1:, 0] = np.where(rng.random(X * Y - 1) < 0.5, rows[:-1, -1], rows[1:, 0])
    assert (lab > max_label).any() and ((lab > 0) & (lab <= max_label)).any()
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(zl), indexing="ij")
    gidx = ((x * Y + y) * Zg + z_off + z).astype(np.int64)
    want = np.full(max_label + 1 + 150, 0xFFFFFFFF, dtype=np.int64)      # 150 entries past max_label: never touched
    keep = (lab > 0) & (lab <= max_label)
    np.minimum.at(want, lab[keep], gidx[keep])
    assert (want[1:max_label + 1] == 0xFFFFFFFF).any()                   # some ids do not occur
    first = torch.full((max_label + 1 + 150,), -1, dtype=torch.int32, device=dev)
    lab_d = _i32(lab)
    _ffi.check(_ffi.lib.sk_first_seen(_ffi.ptr(lab_d), X, Y, zl, z_off, Zg, max_label, _ffi.ptr(first), _ffi.stream_ptr(dev)))
    torch.cuda.synchronize()
    got = first.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(got, want)
