"""The resident JPEG store on the GPU (include/fear_train.h: fear_jpeg_index_build, fear_jpeg_huffman_indexed; DESIGN.md section 14, "The
resident store"): the index through the C ABI against jpeg_huffman.jpeg_scan_index_host with `==`; the indexed decode against the host
library's fear_jpeg_entropy_decode — the same coefficients in one ragged call and one by one at three subsequence lengths, and Pillow's
recorded pixels through the unchanged fear_jpeg_decode_u8; the host library's verdict on every flipped byte and every prefix; the
argument checks of both calls; and `JpegStore` against `JpegDecoder`."""
import ctypes

import numpy as np
import pytest
import torch

import jpegdec
import jpeghuff
from dataops import GUARD, P, SENTINEL_U8, equal as _equal, guarded, inner, inside
from jpegdec import ERR_FORMAT, ERR_NULL, ERR_SHAPE, OK
from feartracker_amd import JpegDecoder, JpegStore, MalformedJPEG, StoreFull, UnsupportedJPEG, jpeg_scan_index_host
from feartracker_amd import train_abi as abi
from feartracker_amd.jpeg_huffman import SUBSEQ_DTYPE, scan_sub_start

pytestmark = pytest.mark.gpu
RECORD = ctypes.sizeof(abi.FearJpegScan)


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


@pytest.fixture(scope="module")
def sequential(lib):
    """{name: the unpacked output of fear_jpeg_entropy_decode} for every supported file, computed once and shared."""
    return {name: jpegdec.unpack(*jpegdec.c_decode(lib, data)) for name, data, _ in jpeghuff.supported()}


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


class _Built:
    """One fear_jpeg_index_build call over `files` and what it left on the device: the scans as fear_jpeg_huffman takes them, one guarded
    buffer for all indexes, the sub_start tables, and the records of both tables."""

    def __init__(self, lib, files, subsequence_bytes, run=True):
        self.lib, self.sb = lib, subsequence_bytes
        self.prepared = [jpeghuff.c_prepare(lib, data) for data in files]
        assert not any(isinstance(p, int) for p in self.prepared)
        n = self.n = len(self.prepared)
        self.records, host, at, self.table_at, self.records_at, self.values = jpeghuff.huffman_layout(self.prepared)
        self.up = torch.empty(host.nbytes, dtype=torch.uint8, device="cuda")
        jpeghuff.finish_layout(self.records, host, at, self.table_at, self.records_at, self.up.data_ptr())
        self.up.copy_(torch.from_numpy(host))
        self.infos = [p[0] for p in self.prepared]
        self.seg = [np.ascontiguousarray(p[2]) for p in self.prepared]
        self.sub = [scan_sub_start(seg, subsequence_bytes) for seg in self.seg]
        self.n_sub = [int(s[-1]) for s in self.sub]
        self.index_at = np.concatenate([[0], np.cumsum(self.n_sub)]).astype(np.int64)
        self.index = guarded(16 * int(self.index_at[-1]))
        sub_at, flat = [], []
        for s in self.sub:
            sub_at.append(4 * sum(f.size for f in flat))
            flat.append(np.concatenate([s, np.zeros(-s.size % 4, np.uint32)]))
        self.sub_dev = torch.from_numpy(np.concatenate(flat)).cuda()
        self.indexes = (abi.FearJpegIndex * n)()
        for k in range(n):
            ix = self.indexes[k]
            ix.index = self.index.data_ptr() + GUARD + 16 * int(self.index_at[k])
            ix.sub_start, ix.seg_start_host, ix.n_sub = self.sub_dev.data_ptr() + sub_at[k], self.seg[k].ctypes.data, self.n_sub[k]
        self.index_table = torch.from_numpy(np.frombuffer(self.indexes, dtype=np.uint8).copy()).cuda()
        self.coef = guarded(2 * self.values)
        self.status = torch.full((n + 2,), 77, dtype=torch.int32, device="cuda")
        if run:
            assert self.call() == OK
            torch.cuda.synchronize()

    def call(self, n=None, **kw):
        a = dict(scans=self.records, table=P(self.up.data_ptr() + self.table_at), indexes=self.indexes, index_table=P(self.index_table.data_ptr()),
                 out=inner(self.coef), st=P(self.status.data_ptr()), sb=self.sb)
        a.update(kw)
        return self.lib.fear_jpeg_index_build(a["scans"], self.n if n is None else n, a["table"], a["indexes"], a["index_table"], a["out"],
                                              a["st"], a["sb"], _stream())

    def statuses(self):
        st = self.status.cpu().numpy()
        assert st[self.n] == 77 and st[self.n + 1] == 77, "a status behind the last image written"
        return st[:self.n]

    def entries(self):
        flat = inside(self.index, 16 * int(self.index_at[-1]), "index").view(SUBSEQ_DTYPE)
        return [flat[self.index_at[k]:self.index_at[k + 1]] for k in range(self.n)]

    def dense(self):
        flat = inside(self.coef, 2 * self.values, "coefficients").view(np.int16)
        return [flat[self.records[k].coef_offset:self.records[k].coef_offset + 64 * self.infos[k].total_blocks] for k in range(self.n)]


class _Indexed:
    """One fear_jpeg_huffman_indexed call over the images `which` of a built index, in that order."""

    def __init__(self, built, which, run=True):
        self.built, self.which, m = built, list(which), len(which)
        self.m = m
        self.images = (abi.FearJpegIndexed * m)()
        prefix, self.values = np.zeros(m + 1, dtype=np.uint32), 0
        for j, k in enumerate(self.which):
            im, ix = self.images[j], built.indexes[k]
            im.scan = built.up.data_ptr() + built.table_at + built.records_at + RECORD * k
            im.index, im.sub_start, im.n_sub, im.coef_offset = ix.index, ix.sub_start, ix.n_sub, self.values
            self.values += 64 * built.infos[k].total_blocks
            prefix[j + 1] = prefix[j] + -(-ix.n_sub // 256)
        self.groups = prefix
        records_at = (4 * m + 4 + 15) & ~15
        table = np.zeros(records_at + ctypes.sizeof(self.images), dtype=np.uint8)
        table[:prefix.nbytes] = prefix.view(np.uint8)
        table[records_at:] = np.frombuffer(self.images, dtype=np.uint8)
        self.table = torch.from_numpy(table).cuda()
        self.coef = guarded(2 * self.values)
        self.status = torch.full((m + 2,), 77, dtype=torch.int32, device="cuda")
        if run:
            assert self.call() == OK
            torch.cuda.synchronize()

    def call(self, n=None, **kw):
        a = dict(images=self.images, table=P(self.table.data_ptr()), out=inner(self.coef), st=P(self.status.data_ptr()), sb=self.built.sb)
        a.update(kw)
        return self.built.lib.fear_jpeg_huffman_indexed(a["images"], self.m if n is None else n, a["table"], a["out"], a["st"], a["sb"], _stream())

    def statuses(self):
        st = self.status.cpu().numpy()
        assert st[self.m] == 77 and st[self.m + 1] == 77, "a status behind the last image written"
        return st[:self.m]

    def dense(self):
        flat = inside(self.coef, 2 * self.values, "coefficients").view(np.int16)
        return [flat[self.images[j].coef_offset:self.images[j].coef_offset + 64 * self.built.infos[k].total_blocks]
                for j, k in enumerate(self.which)]

    def pixels(self):
        """The unchanged fear_jpeg_decode_u8 on the dense coefficients still on the device, every record at the shared block_start table."""
        lib, infos = self.built.lib, [self.built.infos[k] for k in self.which]
        dummy = (np.zeros(1, np.int16), np.zeros(1, np.uint32))
        records, jinfos, prefix, at, _, out_bytes = jpegdec.call_layout([(info,) + dummy for info in infos])
        most = max(info.total_blocks for info in infos)
        start = torch.empty(most + 1, dtype=torch.int32, device="cuda")
        assert lib.fear_jpeg_dense_block_start(P(start.data_ptr()), most, _stream()) == OK
        out, ws_bytes = guarded(out_bytes), lib.fear_jpeg_decode_workspace_bytes(jinfos, self.m)
        ws = guarded(ws_bytes)
        for j in range(self.m):
            records[j].coef = self.coef.data_ptr() + GUARD + 2 * self.images[j].coef_offset
            records[j].block_start = start.data_ptr()
            records[j].out = out.data_ptr() + GUARD + at["out"][j]
        table = torch.from_numpy(jpegdec.table_bytes(prefix, records)).cuda()
        assert lib.fear_jpeg_decode_u8(records, self.m, P(table.data_ptr()), inner(ws), ws_bytes, _stream()) == OK
        torch.cuda.synchronize()
        inside(ws, ws_bytes, "workspace")
        flat = inside(out, out_bytes)
        return [flat[at["out"][j]:at["out"][j] + i.height * i.width * 3].reshape(i.height, i.width, 3) for j, i in enumerate(infos)]


def _check_coefficients(names, infos, dense, sequential, what):
    for name, info, flat in zip(names, infos, dense):
        for c, (a, b) in enumerate(zip(jpeghuff.dense(info, flat), sequential[name])):
            assert a.shape == b.shape and bool((a == b).all()), f"{what} {name}: component {c}: {int((a != b).sum())} values differ"


@pytest.fixture(scope="module")
def built(lib):
    """{subsequence_bytes: the index of every supported file, built in one ragged call}, built once and shared."""
    files = [data for _, data, _ in jpeghuff.supported()]
    return {sb: _Built(lib, files, sb) for sb in (4, 16, 128)}


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_index_build_equals_the_host_index(lib, built, sequential, subsequence_bytes):
    cases, b = jpeghuff.supported(), built[subsequence_bytes]
    status = b.statuses()
    assert not status.any(), [(cases[k][0], int(status[k])) for k in np.flatnonzero(status)]
    files = [data for _, data, _ in cases]
    prepared = [jpeghuff.c_prepare(lib, data) for data in files]                       # fear_jpeg_huffman on the same files: the same verdicts
    records, host, at, table_at, records_at, values = jpeghuff.huffman_layout(prepared)
    up = torch.empty(host.nbytes, dtype=torch.uint8, device="cuda")
    jpeghuff.finish_layout(records, host, at, table_at, records_at, up.data_ptr())
    up.copy_(torch.from_numpy(host))
    coef, plain = guarded(2 * values), torch.full((len(files),), 77, dtype=torch.int32, device="cuda")
    assert lib.fear_jpeg_huffman(records, len(files), P(up.data_ptr() + table_at), inner(coef), P(plain.data_ptr()), subsequence_bytes, _stream()) == OK
    torch.cuda.synchronize()
    assert np.array_equal(plain.cpu().numpy(), status)
    assert np.array_equal(inside(coef, 2 * values), inside(b.coef, 2 * b.values))       # and the same coefficients, value for value
    _check_coefficients([c[0] for c in cases], b.infos, b.dense(), sequential, f"{subsequence_bytes} bytes, scratch of the build:")
    for (name, data, _), got, sub in zip(cases, b.entries(), b.sub):
        _, sub_start, index, want = jpeg_scan_index_host(data, subsequence_bytes)
        assert want == 0 and np.array_equal(sub, sub_start), name
        assert got.shape == index.shape and got.tobytes() == index.tobytes(), f"{name}: {int((got != index).sum())} entries differ"


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_indexed_decode_of_every_file_in_one_ragged_call(built, sequential, subsequence_bytes):
    """At 4 bytes the 51 kB file spans more than 40 workgroups and the 13 kB one 14; the rst3 files have segments shorter than one
    subsequence and many of them in one workgroup; 1x1 has one block."""
    cases, b = jpeghuff.supported(), built[subsequence_bytes]
    order = list(range(len(cases)))[::-1]                                               # another order than the build's
    run = _Indexed(b, order)
    if subsequence_bytes == 4:
        per_image = np.diff(run.groups)
        assert per_image.max() > 40 and (per_image >= 12).sum() >= 2 and per_image.min() == 1
    status = run.statuses()
    assert not status.any(), [(cases[order[j]][0], int(status[j])) for j in np.flatnonzero(status)]
    _check_coefficients([cases[k][0] for k in order], [b.infos[k] for k in order], run.dense(), sequential, f"{subsequence_bytes} bytes")
    for got, k in zip(run.pixels(), order):
        assert got.shape == cases[k][2].shape and np.array_equal(got, cases[k][2]), f"{cases[k][0]}: pixels differ from Pillow's"


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_indexed_decode_of_every_file_on_its_own(built, sequential, subsequence_bytes):
    cases, b = jpeghuff.supported(), built[subsequence_bytes]
    for k, case in enumerate(cases):
        run = _Indexed(b, [k])
        assert run.statuses()[0] == OK, case[0]
        _check_coefficients([case[0]], [b.infos[k]], run.dense(), sequential, f"{subsequence_bytes} bytes, alone:")
    assert np.array_equal(run.pixels()[0], case[2])                                     # (the last file through the pixel stage alone)


def test_hostile_corpus_through_build_and_indexed_decode(lib):
    """Every flipped entropy byte and every prefix of the 16 x 16 4:2:0 file that gets as far as the device, in one ragged call each:
    the build's status and the indexed decode's are fear_jpeg_entropy_decode's, and its coefficients where it accepts."""
    files, want = [], []
    for what, data in jpeghuff.corpus():
        if isinstance(jpeghuff.c_prepare(lib, data), int):
            continue
        files.append((what, data))
        want.append(jpegdec.c_decode(lib, data))
    assert len(files) > 1000
    for subsequence_bytes in (4, 128):
        b = _Built(lib, [data for _, data in files], subsequence_bytes)
        run = _Indexed(b, range(len(files)))
        first, second, dense, accepted = b.statuses(), run.statuses(), run.dense(), 0
        b.entries()                                                                    # (the guard bands of the index)
        for k, ((what, _), ref) in enumerate(zip(files, want)):
            verdict = ref if isinstance(ref, int) else OK
            assert first[k] == verdict and second[k] == verdict, f"{what}: build {first[k]}, indexed {second[k]}, host {verdict}"
            if not isinstance(ref, int):
                accepted += 1
                for a, c in zip(jpeghuff.dense(b.infos[k], dense[k]), jpegdec.unpack(*ref)):
                    assert bool((a == c).all()), what
        assert 100 < accepted < len(files) - 100
        assert set(np.unique(second)) == {OK, ERR_FORMAT}


def test_argument_checks_of_both_calls(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    b = _Built(lib, [data], 128, run=False)
    ix = b.indexes[0]

    def with_field(record, call, **fields):
        saved = {k: getattr(record, k) for k in fields}
        for k, v in fields.items():
            setattr(record, k, v)
        rc = call()
        for k, v in saved.items():
            setattr(record, k, v)
        return rc

    assert b.call(n=0, scans=None, table=None, indexes=None, index_table=None, out=None, st=None) == OK
    assert b.call(n=-1) == ERR_SHAPE and b.call(n=65536) == ERR_SHAPE
    for sb in (0, 2, 6, 130, 1028, -128):
        assert b.call(sb=sb) == ERR_SHAPE, sb
    for name in ("scans", "table", "indexes", "index_table", "out", "st"):
        assert b.call(**{name: None}) == ERR_NULL, name
    assert with_field(b.records[0], b.call, bytes=0) == ERR_NULL and with_field(b.records[0], b.call, seg_start=0) == ERR_NULL
    assert with_field(b.records[0], b.call, n_seg=b.records[0].n_seg + 1) == ERR_SHAPE      # fear_jpeg_huffman's own checks hold
    assert with_field(b.records[0], b.call, bytes=b.records[0].bytes + 1) == ERR_SHAPE
    for null in ("index", "sub_start", "seg_start_host"):
        assert with_field(ix, b.call, **{null: 0}) == ERR_NULL, null
    assert with_field(ix, b.call, index=ix.index + 8) == ERR_SHAPE and with_field(ix, b.call, sub_start=ix.sub_start + 2) == ERR_SHAPE
    assert with_field(ix, b.call, n_sub=ix.n_sub - 1) == ERR_SHAPE and with_field(ix, b.call, n_sub=ix.n_sub + 1) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((inside(b.coef, 2 * b.values) == SENTINEL_U8).all()) and bool((inside(b.index, 16 * ix.n_sub) == SENTINEL_U8).all())
    assert int(b.status[0]) == 77                                                      # none of the refused calls launched anything
    assert b.call() == OK
    torch.cuda.synchronize()
    assert b.statuses()[0] == OK
    assert b.entries()[0].tobytes() == jpeg_scan_index_host(data, 128)[2].tobytes()

    run = _Indexed(b, [0], run=False)
    im = run.images[0]
    assert run.call(n=0, images=None, table=None, out=None, st=None) == OK
    assert run.call(n=-1) == ERR_SHAPE and run.call(n=65536) == ERR_SHAPE
    for sb in (0, 2, 6, 130, 1028, -128):
        assert run.call(sb=sb) == ERR_SHAPE, sb
    for name in ("images", "table", "out", "st"):
        assert run.call(**{name: None}) == ERR_NULL, name
    for null in ("scan", "index", "sub_start"):
        assert with_field(im, run.call, **{null: 0}) == ERR_NULL, null
    assert with_field(im, run.call, index=im.index + 8) == ERR_SHAPE and with_field(im, run.call, sub_start=im.sub_start + 2) == ERR_SHAPE
    assert with_field(im, run.call, scan=im.scan + 4) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((inside(run.coef, 2 * run.values) == SENTINEL_U8).all()) and int(run.status[0]) == 77
    assert run.call() == OK
    torch.cuda.synchronize()
    assert run.statuses()[0] == OK
    ref = jpegdec.unpack(*jpegdec.c_decode(lib, data))
    for a, c in zip(jpeghuff.dense(b.infos[0], run.dense()[0]), ref):
        assert bool((a == c).all())


def without_lanes(run, **fields):
    """The call of `run`, of one image and not yet run, with `fields` of its record set on the host and in the device table and no
    workgroup in the prefix table — what a call sees whose images leave it no lane to run: OK, the statuses written, nothing stored.
    The image's status."""
    for k, v in fields.items():
        setattr(run.images[0], k, v)
    table = run.table.cpu().numpy()
    table[:8] = 0
    table[16:] = np.frombuffer(run.images, dtype=np.uint8)                             # one image: the records begin at 16
    run.table = torch.from_numpy(table).cuda()
    assert run.call() == OK
    torch.cuda.synchronize()
    assert bool((inside(run.coef, 2 * run.values) == SENTINEL_U8).all())
    return run.statuses()[0]


def test_an_image_without_a_subsequence_has_no_lane_and_fails(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    assert without_lanes(_Indexed(_Built(lib, [data], 128), [0], run=False), n_sub=0) == ERR_FORMAT


# ------------------------------------------------------------------------------------------------------------------------- JpegStore
@pytest.fixture(scope="module")
def host_frames():
    """JpegDecoder's host-mode frames of every supported file, decoded once and left unchanged."""
    dec = JpegDecoder(device=0, threads=4)
    frames = dec.decode([data for _, data, _ in jpeghuff.supported()])
    torch.cuda.synchronize()
    dec.close()
    return frames


def _same_frames(frames, ids, host_frames, cases):
    for f, i in zip(frames, ids):
        name, _, px = cases[int(i)]
        assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() and torch.equal(f, host_frames[int(i)]), name
        assert np.array_equal(f.cpu().numpy(), px), name


@pytest.mark.parametrize("subsequence_bytes, slab_bytes", [(4, 4096), (128, 4096), (16, 40_000)])
def test_store_frames_equal_the_decoders(host_frames, subsequence_bytes, slab_bytes):
    """A file's FearJpegScan record alone is 8704 bytes: at 4096 every file has a slab of its own; at 40 000 several share one and the
    largest still exceed it."""
    cases = jpeghuff.supported()
    files = [data for _, data, _ in cases]
    store = JpegStore(device=0, subsequence_bytes=subsequence_bytes, slab_bytes=slab_bytes, threads=4, initial_rows=4)
    try:
        first = store.add(files[:20])
        one = store.decode(first[:3], check=True)                                      # before the mirrors grow again
        ids = np.concatenate([first, store.add(files[20:])])
        assert ids.dtype == np.int64 and ids.tolist() == list(range(len(files))) and len(store) == len(files)
        own = sum(s.numel() > slab_bytes for s in store._slabs)                         # many slabs, files above a slab
        assert (own == len(files) == len(store._slabs)) if slab_bytes == 4096 else (0 < own < 10 and own + 5 < len(store._slabs) < len(files) - 5)
        assert set(store.kinds) == {"scan"} and store.nbytes == sum(store.resident.values()) > sum(len(f) for f in files) // 2
        assert store.shape(ids).tolist() == [list(px.shape[:2]) for _, _, px in cases]
        _same_frames(one, first[:3], host_frames, cases)
        _same_frames(store.decode(ids), ids, host_frames, cases)
        _same_frames(store.decode(ids[::-1]), ids[::-1], host_frames, cases)
        again = np.array([5, 5, 50, 0, 5, 17, 50])
        _same_frames(store.decode(again), again, host_frames, cases)
        for i in ids:
            _same_frames(store.decode([i]), [i], host_frames, cases)
        frames = store.decode(ids)
        for f in frames:
            f.fill_(7)                                                                 # a frame is private: the store does not see this
        _same_frames(store.decode(ids, check=True), ids, host_frames, cases)
        assert store.decode([]) == []
        store.check()                                                                  # nothing pending: returns
    finally:
        store.close()


def test_store_decode_never_waits_for_the_gpu(host_frames):
    cases = jpeghuff.supported()
    store = JpegStore(device=0, threads=4)
    try:
        ids = store.add([data for _, data, _ in cases])
        store.decode(ids[:3], check=True)                                              # (the allocators warm)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            frames = store.decode(ids[::-1])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        store.check()
        _same_frames(frames, ids[::-1], host_frames, cases)
    finally:
        store.close()


def test_store_faults_and_kinds(monkeypatch):
    from feartracker_amd import jpeg_frames
    name, good, px = jpegdec.case("16x16_420")
    cut = good[:len(good) - 40]                                                        # the headers are whole, the entropy data is not
    other = jpegdec.case("80x72_420")
    store = JpegStore(device=0, slab_bytes=40_000, threads=2)
    try:
        ids = store.add([good, other[1]])
        before = (len(store), store.nbytes, len(store._slabs), store._cursor)
        with pytest.raises(MalformedJPEG, match="item 1"):
            store.add([good, cut, good])
        assert (len(store), store.nbytes, len(store._slabs), store._cursor) == before
        launched = []
        real = abi.launch
        monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
        with pytest.raises(MalformedJPEG, match="item 1"):
            store.add([good, good[:400]], fallback=lambda data: np.zeros((16, 16, 3), np.uint8))
        rst = next(data for name, data, _ in jpegdec.supported() if "rst3" in name and data.count(b"\xff\xd1") == 1)
        with pytest.raises(MalformedJPEG, match="restart marker"):
            store.add([good, rst.replace(b"\xff\xd1", b"\xff\xd2")])                    # a marker fault is the host's to find
        with pytest.raises(IndexError):
            store.decode([0, 2])
        with pytest.raises(IndexError):
            store.decode([-1])
        assert launched == [] and (len(store), store.nbytes) == before[:2]
        frames = store.decode(ids, check=True)
        assert launched == ["fear_jpeg_dense_block_start", "fear_jpeg_huffman_indexed", "fear_jpeg_decode_u8"]
        assert np.array_equal(frames[0].cpu().numpy(), px) and np.array_equal(frames[1].cpu().numpy(), other[2])
        store.decode(ids[:1], check=True)                                              # the largest image did not grow: no block_start launch
        assert launched[3:] == ["fear_jpeg_huffman_indexed", "fear_jpeg_decode_u8"]
        # a progressive file
        prog = jpegdec.case("33x31_420_smooth_q75_progressive")
        with pytest.raises(UnsupportedJPEG, match="progressive"):
            store.add([good, prog[1]])
        assert (len(store), store.nbytes) == before[:2]
        seen = []

        def fallback(data):
            seen.append(data)
            return prog[2]

        more = store.add([good, prog[1], other[1]], fallback=fallback)
        assert seen == [prog[1]] and store.kinds[more].tolist() == ["scan", "pixels", "scan"]
        mixed = store.decode(more[::-1], check=True)
        for f, ref in zip(mixed, (other[2], prog[2], px)):
            assert np.array_equal(f.cpu().numpy(), ref)
        mixed[1].fill_(0)
        assert np.array_equal(store.decode(more[1:2])[0].cpu().numpy(), prog[2])         # a copy, never the store's own pixels
    finally:
        store.close()
    # a restart segment above the device's limit is decoded once on the host and kept as pixels (the limit lowered for the test)
    cases = jpeghuff.entropy_cases()[:4]
    monkeypatch.setattr(jpeg_frames, "DEVICE_SCAN_MAX", 10_000)                        # two of the four files are longer
    store = JpegStore(device=0, threads=2)
    try:
        ids = store.add([data for _, data, _ in cases])
        assert sorted(store.kinds) == ["pixels", "pixels", "scan", "scan"]
        for f, (name, _, ref) in zip(store.decode(ids, check=True), cases):
            assert np.array_equal(f.cpu().numpy(), ref), name
    finally:
        store.close()


def test_an_add_the_device_refuses_commits_nothing(lib):
    """`add` assigns to the store in its last stage alone: after a call whose second file the device refuses (a status of
    fear_jpeg_index_build, by when the call's first file is uploaded and indexed) the store is what it was, and the next call goes on
    from there."""
    first, second, good = jpegdec.case("16x16_420"), jpegdec.case("80x72_420"), jpegdec.case("15x50_420_random_q100_rst3")
    refused = next(data for _, data in jpeghuff.corpus()
                   if not isinstance(jpeghuff.c_prepare(lib, data), int) and isinstance(jpegdec.c_decode(lib, data), int))
    store, dec = JpegStore(device=0, slab_bytes=40_000, threads=2), JpegDecoder(device=0, threads=2)

    def state():
        return len(store), store.nbytes, dict(store.resident), store.kinds.tolist(), store.borders([0, 1]).cpu().tolist()
    try:
        ids = store.add([first[1], second[1]])
        frames = [f.clone() for f in store.decode(ids, check=True)]
        before = state()
        with pytest.raises(MalformedJPEG, match="^item 1: "):
            store.add([good[1], refused])
        assert state() == before and before[0] == 2
        again = store.decode([0, 1], check=True)
        assert all(torch.equal(f, was) for f, was in zip(again, frames)) and np.array_equal(again[1].cpu().numpy(), second[2])
        more = store.add([good[1]])
        assert more.tolist() == [2] and len(store) == 3 and store.kinds.tolist() == ["scan"] * 3
        frame = store.decode(more, check=True)[0]
        assert torch.equal(frame, dec.decode([good[1]])[0]) and np.array_equal(frame.cpu().numpy(), good[2])
    finally:
        store.close()
        dec.close()


def test_store_capacity():
    files = [data for _, data, _ in jpegdec.supported()[:6]]
    store = JpegStore(device=0, slab_bytes=40_000, threads=2)
    store.add(files[:3])
    store.add(files[3:])
    total = store.nbytes
    store.close()
    store = JpegStore(device=0, slab_bytes=40_000, threads=2, capacity_bytes=total - 1)
    try:
        ids = store.add(files[:3])
        before = (len(store), store.nbytes, len(store._slabs), store._cursor)
        with pytest.raises(StoreFull):
            store.add(files[3:])
        assert isinstance(StoreFull("x"), MemoryError) and (len(store), store.nbytes, len(store._slabs), store._cursor) == before
        store.capacity_bytes = total
        assert store.add(files[3:]).tolist() == [3, 4, 5] and store.nbytes == total
        for f, (_, _, px) in zip(store.decode(np.arange(6), check=True), jpegdec.supported()[:6]):
            assert np.array_equal(f.cpu().numpy(), px)
    finally:
        store.close()


def test_a_tiny_workspace_limit_splits_the_stores_call(monkeypatch):
    cases = jpeghuff.entropy_cases() + jpegdec.supported()[::5]
    files = [data for _, data, _ in cases]
    stores = [JpegStore(device=0, threads=2, workspace_limit=limit) for limit in (1 << 30, 300_000, 1)]
    try:
        launched = []
        real = abi.launch
        monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
        counts, results = [], []
        for store in stores:
            ids = store.add(files)
            del launched[:]
            results.append(store.decode(ids, check=True))
            counts.append(launched.count("fear_jpeg_huffman_indexed"))
            assert counts[-1] == launched.count("fear_jpeg_decode_u8")
        assert counts[0] == 1 and 4 <= counts[1] < len(files) and counts[2] == len(files)   # a 256 x 192 4:4:4 file needs 294 912 bytes dense
        for whole, (_, _, px) in zip(results[0], cases):
            assert np.array_equal(whole.cpu().numpy(), px)
        for parts in results[1:]:
            for x, y in zip(results[0], parts):
                assert torch.equal(x, y)
    finally:
        for store in stores:
            store.close()


def test_train_pairs_from_store_decoded_frames():
    from feartracker_amd.train_data import TrainPairBuilder
    cases = [jpegdec.case("64x48_444_random_q100_plain2"), jpegdec.case("80x72_420"), jpegdec.case("64x48_gray"), jpegdec.case("80x72_422")]
    B = 4
    rng = np.random.default_rng(3)
    pairs = np.zeros((B, 11))
    for k in range(B):
        for col, f in ((0, k % 4), (5, (k + 1) % 4)):
            h, w = cases[f][2].shape[:2]
            bw, bh = rng.integers(8, w // 2), rng.integers(8, h // 2)
            pairs[k, col:col + 5] = [f, rng.integers(0, w - bw + 1), rng.integers(0, h - bh + 1), bw, bh]
        pairs[k, 10] = 1
    builder = TrainPairBuilder(device=0)
    params = builder.draw(pairs, [c[2].shape[:2] for c in cases], np.random.default_rng(7))
    store = JpegStore(device=0, threads=2)
    try:
        frames = store.decode(store.add([c[1] for c in cases]), check=True)
        dev = builder.build(frames, pairs, params)
        ref = builder.build([np.ascontiguousarray(c[2]) for c in cases], pairs, params)
        torch.cuda.synchronize()
        _equal(dev, ref)
    finally:
        store.close()
