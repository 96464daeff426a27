"""A scale per position in one `JpegStore` call on the GPU (include/fear_train.h: fear_jpeg_decode_mixed_u8; DESIGN.md section 14, "A
scale per position"): item i of a mixed `decode`, `decode_rows` or `decode_windows` against the uniform call at its own scale, byte for
byte, over the fixture files of all four modes; the entry point through the C ABI against the recorded pixels, with its argument checks
and a guard band around the workspace and every frame."""
import numpy as np
import pytest
import torch

import jpegdec
import jpegscaled
from dataops import GUARD, P, SENTINEL_U8, guarded, inner, inside
from jpegdec import ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, OK
from feartracker_amd import JpegStore, UnsupportedJPEG, jpeg_scaled_shape
from feartracker_amd import train_abi as abi

pytestmark = pytest.mark.gpu
ALL = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


@pytest.fixture(scope="module")
def store():
    """The fixture files of all four modes, the progressive twin as a transcoded scan entry, and the reference every test shares:
    `decode([id], scale=s)[0]` per file and scale, computed once and left unchanged."""
    files = jpegscaled.files(progressive=True)
    s = JpegStore(device=0, threads=4, progressive=True)
    ids = s.add([data for _, data in files])
    assert (s.kinds[ids] == "scan").all() and "progressive" in files[-1][0]
    modes = {name.split("_")[1] for name, _ in files}
    assert modes == {"444", "422", "420", "gray"}
    one = {(k, sc): s.decode([ids[k]], scale=sc)[0] for k in range(len(files)) for sc in ALL}
    s.check()
    yield s, files, ids, one
    s.close()


def _launched(monkeypatch):
    names = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: names.append(name) or real(lib, name, *args))
    return names


def _check(frames, which, scales, one, files):
    assert len(frames) == len(which)
    for pos, (f, k, sc) in enumerate(zip(frames, which.tolist(), scales.tolist())):
        want = one[(k, sc)]
        assert f.shape == want.shape and torch.equal(f, want), f"position {pos}: {files[k][0]} at 1/{sc}"


def _pixels(files_shapes, k, sc):
    h, w, _ = jpeg_scaled_shape(*files_shapes[k], sc)
    return h * w


def test_mixed_decode_equals_the_uniform_decode_item_by_item(store, monkeypatch):
    s, files, ids, one = store
    n = len(files)
    rng = np.random.default_rng(1)
    shapes = [tuple(x) for x in s.shape(ids).tolist()]
    names = _launched(monkeypatch)

    def run(which, scales, mixed=True):
        which, scales = np.asarray(which), np.asarray(scales)
        del names[:]
        frames = s.decode(ids[which], check=True, scale=scales)
        assert ("fear_jpeg_decode_mixed_u8" in names) == mixed, names
        _check(frames, which, scales, one, files)
        assert np.array_equal(s.shape(ids[which], scales), [f.shape[:2] for f in frames])

    # every file at all four scales in one call, shuffled
    which, scales = np.repeat(np.arange(n), 4), np.tile(ALL, n)
    order = rng.permutation(which.size)
    run(which[order], scales[order])
    # neighbours in the table always differ in scale, both ways round
    run(np.arange(n), np.array(ALL)[np.arange(n) % 4])
    run(np.arange(n)[::-1], np.array(ALL[::-1])[np.arange(n) % 4])
    # the same id four times
    for k in (0, 22, n - 1):
        run([k] * 4, [8, 1, 4, 2])
    # n = 1: a sequence of one scale takes the uniform launch, as every sequence of equal values does
    for sc in ALL:
        run([38], [sc], mixed=False)
        run([3, 38, 46], (sc, sc, sc), mixed=False)
    # the 1 x 1 files and the files smaller than the scale (7 x 5 at 1/8), next to full-size neighbours
    tiny = [k for k in range(n) if shapes[k][0] * shapes[k][1] <= 35]
    assert len(tiny) == 8
    run(np.repeat(tiny, 2), np.tile([8, 1], len(tiny)))
    run(np.repeat(tiny, 2), np.tile([2, 4], len(tiny)))
    # files under and over 256 scaled pixels next to each other: the steps of the pixel prefix table are 1 and more than 1
    pick = [(k, sc) for k in range(n) for sc in ALL]
    over = [p for p in pick if _pixels(shapes, *p) > 256]
    under = [p for p in pick if _pixels(shapes, *p) <= 256]
    under = [under[i] for i in rng.permutation(len(under))[:len(over)]]
    assert len(under) == len(over) >= 40 and {sc for _, sc in under} == set(ALL) and {sc for _, sc in over} >= {1, 2, 4}
    both = [p for pair in zip(under, over) for p in pair]
    run([k for k, _ in both], [sc for _, sc in both])
    # the 4:2:2 files at the cw <= 2 threshold: scaled chroma planes 3 and 2 wide, and the full-size plane above it
    edge = [k for k, (name, _) in enumerate(files) if "_cw3" in name or name.startswith(("1x1_422", "7x5_422"))]
    assert len(edge) == 4
    run(np.repeat(edge, 4), np.tile([1, 2, 4, 8], len(edge)))
    run(np.repeat(edge, 4), np.tile([8, 4, 2, 1], len(edge)))


def test_a_call_cut_into_groups_whose_scales_differ(store, monkeypatch):
    s, files, ids, one = store
    small = JpegStore(device=0, threads=2, workspace_limit=128 * 40, progressive=True)
    try:
        few = np.arange(28, 48)
        mine = small.add([files[k][1] for k in few])
        scales = np.array([1, 1, 2, 8, 4, 4, 4, 1, 2, 2, 8, 1, 8, 8, 4, 2, 1, 1, 4, 8])
        from feartracker_amd.jpeg_store import plan_decode
        plans = plan_decode(small._columns, mine, small.workspace_limit, scale=scales)
        kinds = [len(set(p["scales"].tolist())) for p in plans]
        assert len(plans) >= 6 and max(kinds) > 1                                   # several groups, mixed ones among them
        assert len({tuple(sorted(set(p["scales"].tolist()))) for p in plans}) >= 4  # and the groups differ in their scales
        names = _launched(monkeypatch)
        frames = small.decode(mine, check=True, scale=scales)
        # which entry points the call's groups took (not how often): the mixed one, and the uniform ones of the groups of one scale
        assert "fear_jpeg_decode_mixed_u8" in names
        alone = {int(p["scales"][0]) for k, p in zip(kinds, plans) if k == 1}
        assert ("fear_jpeg_decode_u8" in names) == (1 in alone) and ("fear_jpeg_decode_scaled_u8" in names) == bool(alone - {1})
        _check(frames, few, scales, one, files)
    finally:
        small.close()


def test_entries_kept_as_pixels_and_bad_scales(store):
    s, files, ids, one = store
    prog = files[-1][1]
    t = JpegStore(device=0, threads=2)
    try:
        kept = np.full((16, 48, 3), 77, np.uint8)
        mine = t.add([files[20][1], prog, files[38][1]], fallback=lambda data: kept)
        assert t.kinds.tolist() == ["scan", "pixels", "scan"]
        frames = t.decode(mine, check=True, scale=[2, 1, 8])
        assert torch.equal(frames[0], one[(20, 2)]) and torch.equal(frames[2], one[(38, 8)])
        assert np.array_equal(frames[1].cpu().numpy(), kept)
        frames = t.decode_rows(mine, [[0, 5], [3, 4], [1, 2]], check=True, scale=[4, 1, 2])
        assert np.array_equal(frames[1].cpu().numpy(), kept) and torch.equal(frames[2][1:2], one[(38, 2)][1:2])
        got = t.decode_windows(mine, [[0, 5, 0, 5], [3, 9, 2, 7], [1, 2, 0, 3]], check=True, scale=[4, 1, 2])
        assert np.array_equal(got.frames[1].cpu().numpy(), kept[3:9, 2:7]) and got.origin[1].tolist() == [3, 2]
        for call in (lambda: t.decode(mine, scale=[1, 2, 1]), lambda: t.decode_rows(mine, np.zeros((3, 2), int), scale=[1, 4, 1]),
                     lambda: t.decode_windows(mine, np.zeros((3, 4), int), scale=[1, 8, 1])):
            with pytest.raises(UnsupportedJPEG, match=f"id {int(mine[1])} "):
                call()
        for bad in ([1, 2], [1, 3, 1], [1, True, 1], [1.0, 2.0, 1.0]):
            with pytest.raises(ValueError, match="scale"):
                t.decode(mine, scale=bad)
        rows = torch.zeros((3, 2), dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match="scale"):
            t.decode_rows(mine, rows, scale=[1, 2, 1])
        assert len(t.decode_rows(mine, rows, check=True, scale=[1, 1, 1])) == 3      # rows on the device: scale 1 alone
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------------------------ rows and windows
def _bands(H, v_rows, rng, k):
    """A band of a frame of H rows whose MCU rows are v_rows high: its top edge, its bottom edge, interior, whole, empty, overhanging."""
    mid = H // 2
    return ((0, 1), (H - 1, H), (0, H), (mid, min(mid + 2, H)), (mid, mid), (H, H + 5), (-3, 1), (max(H - v_rows - 1, 0), H),
            (0, min(v_rows + 1, H)), tuple(sorted(rng.integers(0, H + 1, 2).tolist())))[k % 10]


def test_mixed_decode_rows_equals_the_uniform_rows(store, monkeypatch):
    s, files, ids, one = store
    n = len(files)
    rng = np.random.default_rng(2)
    which, scales, rows = [], [], []
    count = 0
    for k in range(n):
        v = 2 if "_420" in files[k][0] else 1
        for turn in range(10):
            sc = ALL[(k + turn) % 4] if turn < 8 else 1                             # (the last two bands of a file at full size)
            H = one[(k, sc)].shape[0]
            which.append(k)
            scales.append(sc)
            rows.append(_bands(H, v * 8 // sc, rng, 7 if turn == 9 else turn))   # (at full size: a band at the top edge, one at the bottom)
            count += 1
    order = rng.permutation(count)
    which, scales, rows = np.array(which)[order], np.array(scales)[order], np.array(rows)[order]
    names = _launched(monkeypatch)
    frames = s.decode_rows(ids[which], rows, check=True, scale=scales)
    assert "fear_jpeg_decode_mixed_u8" in names and "fear_jpeg_huffman_indexed_rows" in names
    empty = halo_top = halo_bottom = scaled = 0
    for pos, (f, k, sc, (y0, y1)) in enumerate(zip(frames, which.tolist(), scales.tolist(), rows.tolist())):
        want = one[(k, sc)]
        assert f.shape == want.shape
        H = want.shape[0]
        y0, y1 = min(max(y0, 0), H), min(max(y1, 0), H)
        empty += y0 >= y1
        if "_420" in files[k][0] and sc == 1 and y0 < y1 and H > 16:
            halo_top += y0 == 0
            halo_bottom += y1 == H
        scaled += sc > 1 and y0 < y1
        assert torch.equal(f[y0:y1], want[y0:y1]), f"position {pos}: {files[k][0]} at 1/{sc}, rows {y0}..{y1}"
    assert empty > 40 and halo_top > 5 and halo_bottom > 5 and scaled > 100, (empty, halo_top, halo_bottom, scaled)
    # the uniform calls give the same rows: the mixed call against them directly, on the 4:2:0 files
    few = np.flatnonzero(np.array(["_420" in files[k][0] for k in which]))[:40]
    for sc in ALL:
        mine = few[scales[few] == sc]
        uniform = s.decode_rows(ids[which[mine]], rows[mine], check=True, scale=sc)
        for pos, g in zip(mine.tolist(), uniform):
            H = g.shape[0]
            y0, y1 = np.clip(rows[pos], 0, H).tolist()
            assert torch.equal(frames[pos][y0:y1], g[y0:y1])


def test_mixed_decode_windows_equals_the_uniform_windows(store, monkeypatch):
    s, files, ids, one = store
    n = len(files)
    rng = np.random.default_rng(3)
    which, scales, wins = [], [], []
    for k in range(n):
        v = 2 if "_420" in files[k][0] else 1
        for turn in range(8):
            sc = ALL[(k + turn) % 4] if turn < 6 else 1
            H, W = one[(k, sc)].shape[:2]
            y0, y1 = _bands(H, v * 8 // sc, rng, turn)
            x0, x1 = ((0, W), (W - 1, W), (0, 1), (W // 2, W // 2), tuple(sorted(rng.integers(0, W + 1, 2).tolist())))[(k + turn) % 5]
            which.append(k)
            scales.append(sc)
            wins.append((y0, y1, x0, x1))
    order = rng.permutation(len(which))
    which, scales, wins = np.array(which)[order], np.array(scales)[order], np.array(wins)[order]
    names = _launched(monkeypatch)
    got = s.decode_windows(ids[which], wins, check=True, scale=scales)
    assert "fear_jpeg_decode_mixed_u8" in names and "fear_jpeg_huffman_indexed_windows" in names
    assert np.array_equal(got.shape, s.shape(ids[which], scales)) and len(got) == len(which)
    empty = filled = 0
    for pos, (f, k, sc) in enumerate(zip(got.frames, which.tolist(), scales.tolist())):
        want = one[(k, sc)]
        assert got.shape[pos].tolist() == list(want.shape[:2])
        y0, y1, x0, x1 = got.window[pos].tolist()
        H, W = want.shape[:2]
        a0, a1, b0, b1 = wins[pos].tolist()
        clip = (min(max(a0, 0), H), min(max(a1, 0), H), min(max(b0, 0), W), min(max(b1, 0), W))
        if clip[0] >= clip[1] or clip[2] >= clip[3]:
            assert (y0, y1, x0, x1) == (0, 0, 0, 0) and tuple(f.shape) == (0, 0, 3)
            empty += 1
            continue
        assert (y0, y1, x0, x1) == clip
        oy, ox = got.origin[pos].tolist()
        assert torch.equal(f[y0 - oy:y1 - oy, x0 - ox:x1 - ox], want[y0:y1, x0:x1]), f"position {pos}: {files[k][0]} at 1/{sc}, {clip}"
        filled += 1
    assert empty > 30 and filled > 150, (empty, filled)
    for sc in ALL:                                                                   # and against the uniform call itself
        mine = np.flatnonzero(scales == sc)[:25]
        uniform = s.decode_windows(ids[which[mine]], wins[mine], check=True, scale=sc)
        assert np.array_equal(uniform.origin, got.origin[mine]) and np.array_equal(uniform.window, got.window[mine])
        for pos, g in zip(mine.tolist(), uniform.frames):
            y0, y1, x0, x1 = got.window[pos].tolist()
            oy, ox = got.origin[pos].tolist()
            assert g.shape == got.frames[pos].shape
            assert torch.equal(g[y0 - oy:y1 - oy, x0 - ox:x1 - ox], got.frames[pos][y0 - oy:y1 - oy, x0 - ox:x1 - ox])


# ------------------------------------------------------------------------------------------------------------------ through the C ABI
_decoded = {}


def _c_decode(lib, name, data):
    if name not in _decoded:
        _decoded[name] = jpegdec.c_decode(lib, data)
    return _decoded[name]


def _layout(decoded, scales):
    """jpegdec.call_layout with each record's scale in reserved[0] and the second prefix table counting its own scaled pixels; the frames
    keep the full-size gaps between them."""
    records, infos, prefix, at, up_bytes, out_bytes = jpegdec.call_layout(decoded)
    for k, ((info, _, _), sc) in enumerate(zip(decoded, scales)):
        h, w, _ = jpeg_scaled_shape(info.height, info.width, max(sc, 1))
        prefix[1, k + 1] = prefix[1, k] + -(-h * w // abi.FEAR_JPEG_GROUP_PIXELS)
        records[k].reserved[0] = sc
    return records, infos, prefix, at, up_bytes, out_bytes


def _run(lib, files, scales):
    """fear_jpeg_decode_mixed_u8 on the files in one call, the guard bands around the workspace and around every frame checked."""
    decoded = [_c_decode(lib, name, data) for name, data in files]
    n = len(decoded)
    records, infos, prefix, at, up_bytes, out_bytes = _layout(decoded, scales)
    table_at = up_bytes
    host = np.zeros(up_bytes + jpegdec.table_bytes(prefix, records).nbytes, dtype=np.uint8)
    up = torch.empty(host.nbytes, dtype=torch.uint8, device="cuda")
    out = guarded(out_bytes)
    ws_bytes = lib.fear_jpeg_decode_workspace_bytes(infos, n)
    ws = guarded(ws_bytes)
    for k, (info, coef, start) in enumerate(decoded):
        records[k].coef = up.data_ptr() + at["coef"][k]
        records[k].block_start = up.data_ptr() + at["start"][k]
        records[k].out = out.data_ptr() + GUARD + at["out"][k]
        host[at["coef"][k]:at["coef"][k] + coef.nbytes] = coef.view(np.uint8)
        host[at["start"][k]:at["start"][k] + start.nbytes] = start.view(np.uint8)
    host[table_at:] = jpegdec.table_bytes(prefix, records)
    up.copy_(torch.from_numpy(host))
    rc = lib.fear_jpeg_decode_mixed_u8(records, n, P(up.data_ptr() + table_at), inner(ws), ws_bytes, P(torch.cuda.current_stream().cuda_stream))
    assert rc == OK
    torch.cuda.synchronize()
    inside(ws, ws_bytes, "workspace")
    flat = inside(out, out_bytes)
    frames, covered = [], np.zeros(out_bytes, dtype=bool)
    for k, ((info, _, _), sc) in enumerate(zip(decoded, scales)):
        h, w, _ = jpeg_scaled_shape(info.height, info.width, max(sc, 1))
        frames.append(flat[at["out"][k]:at["out"][k] + h * w * 3].reshape(h, w, 3))
        covered[at["out"][k]:at["out"][k] + h * w * 3] = True
    assert np.all(flat[~covered] == SENTINEL_U8), "bytes behind a frame written"
    return frames


def _expected(name, data, sc):
    """Pillow's recorded pixels (at full size: jpeg_decode.npz; the host model for the files the scaled fixture adds)."""
    if sc > 1:
        return jpegscaled.expected(name, data, sc)[0]
    recorded = {n: px for n, _, px in jpegdec.supported()}
    if name not in recorded and ("full", name) not in _decoded:
        from feartracker_amd import jpeg_decode_host
        _decoded[("full", name)] = jpeg_decode_host(data)
    return recorded[name] if name in recorded else _decoded[("full", name)]


def test_c_abi_mixed_call_against_the_recorded_pixels(lib):
    """Every file at the scale its place gives it, twice over so that every file meets every scale; 0 behaves as 1."""
    files = jpegscaled.files()
    for turn in range(5):
        scales = [(1, 2, 4, 8, 0)[(k + turn) % 5] for k in range(len(files))]
        frames = _run(lib, files, scales)
        for got, (name, data), sc in zip(frames, files, scales):
            want = _expected(name, data, sc)
            assert got.shape == want.shape, (name, sc)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{name} at 1/{sc}: {len(bad)} of {want.size} bytes differ, first at {bad[:3].tolist()}"
    for sc in (0, 1, 2, 4, 8):                                                       # n = 1
        one = files[38:39]
        assert np.array_equal(_run(lib, one, [sc])[0], _expected(*one[0], sc))


def test_c_abi_argument_checks(lib):
    name, data, _ = jpegdec.case("17x23_420")
    decoded = [_c_decode(lib, name, data)]
    records, infos, prefix, at, up_bytes, out_bytes = _layout(decoded, [2])
    st = P(torch.cuda.current_stream().cuda_stream)
    up = torch.zeros(up_bytes + 1024, dtype=torch.uint8, device="cuda")
    out = guarded(out_bytes)
    ws_bytes = lib.fear_jpeg_decode_workspace_bytes(infos, 1)
    ws = guarded(ws_bytes)
    table = P(up.data_ptr())

    def call(n=1, images=records, table=table, workspace=inner(ws), nbytes=ws_bytes):
        return lib.fear_jpeg_decode_mixed_u8(images, n, table, workspace, nbytes, st)

    def with_field(**fields):
        saved = {k: getattr(records[0], k) for k in fields}
        for k, v in fields.items():
            setattr(records[0], k, v)
        rc = call()
        for k, v in saved.items():
            setattr(records[0], k, v)
        return rc

    def with_scale(value):
        records[0].reserved[0] = value
        rc = call()
        records[0].reserved[0] = 2
        return rc

    assert call() == ERR_NULL                                                        # the record's pointers are still null
    assert with_scale(3) == ERR_NULL                                                 # the nulls come in front of the shapes
    records[0].coef, records[0].block_start, records[0].out = up.data_ptr(), up.data_ptr(), out.data_ptr() + GUARD
    for bad in (3, -1, 5, 6, 16, -2, 256 + 2, 1 << 16):
        assert with_scale(bad) == ERR_SHAPE, bad
        records[0].reserved[0] = bad
        assert call(workspace=None) == ERR_SHAPE and call(nbytes=0) == ERR_SHAPE     # and the shapes in front of the workspace
        records[0].reserved[0] = 2
    assert call(n=0, images=None, table=None, workspace=None, nbytes=0) == OK
    assert call(n=-1) == ERR_SHAPE and call(n=65536) == ERR_SHAPE
    assert call(images=None) == ERR_NULL and call(table=None) == ERR_NULL
    assert with_field(out=0) == ERR_NULL and with_field(coef=0) == ERR_NULL and with_field(block_start=0) == ERR_NULL
    assert call(workspace=None) == ERR_WORKSPACE and call(nbytes=ws_bytes - 1) == ERR_WORKSPACE and call(nbytes=0) == ERR_WORKSPACE
    assert with_field(plane_offset=16) == ERR_WORKSPACE and with_field(plane_offset=8) == ERR_SHAPE
    for bad in (dict(width=0), dict(height=0), dict(width=8193), dict(components=2), dict(components=4), dict(h=3), dict(h=1, v=2),
                dict(components=1, h=2, v=2)):
        assert with_field(**bad) == ERR_SHAPE, bad
    # reserved[1..2] stay reserved: the checks do not read them
    records[0].reserved[1], records[0].reserved[2] = 3, -1
    assert call(nbytes=ws_bytes - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    inside(ws, ws_bytes, "workspace")
    inside(out, out_bytes)                                                           # none of the refused calls launched anything
