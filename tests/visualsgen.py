"""Deterministic inputs for the drawing and miner tests (test infrastructure): the operator cases that tests/test_visuals_host.py,
tests/test_visuals_gpu.py and tools/visuals_kernel_host_check.py share."""
import numpy as np

THICKNESSES = (1, 2, 5, 32)
FRAME_SHAPES = ((1, 1), (4, 4), (37, 70), (256, 384))


def frame(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def edge_boxes(h: int, w: int) -> np.ndarray:
    """Boxes inside an (h, w) image, touching each edge, with a negative origin, wholly outside, with w or h of 0, negative, and
    smaller than any thickness above 1 (the filled case)."""
    return np.array([
        (w // 4, h // 4, w // 3, h // 3),                   # inside
        (0, 2, 3, 3), (w - 4, 2, 3, 3), (2, 0, 3, 3), (2, h - 4, 3, 3),          # touching the left, right, top, bottom edge
        (0, 0, w - 1, h - 1),                               # the image's own outline
        (-5, -4, 12, 10),                                   # a negative origin
        (w + 40, h + 40, 5, 5), (-100, -100, 10, 10), (w + 16, 2, 4, 4),         # wholly outside (the last by one pixel at t = 32)
        (3, 3, 0, 6), (3, 3, 6, 0), (2, 2, 0, 0),           # w or h of 0
        (w // 2 + 6, h // 2 + 4, -6, -4),                   # negative sides
        (5, 5, 1, 1), (9, 5, 2, 30),                        # thinner than the band
    ], dtype=np.int32)


def colours(k: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, size=(k, 3)).astype(np.uint8)


def random_boxes(k: int, h: int, w: int, seed: int, lo: int = 2, hi: int = 40) -> np.ndarray:
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(-8, w, size=k), rng.randint(-8, h, size=k), rng.randint(lo, hi, size=k),
                     rng.randint(lo, hi, size=k)], axis=1).astype(np.int32)


def draw_cases():
    """(name, [frame shapes], boxes (K, 4), frame_of (K), colours (K, 3), thickness)."""
    for t in THICKNESSES:
        for shape in FRAME_SHAPES:
            b = edge_boxes(*shape)
            yield f"edges {shape} t={t}", [shape], b, np.zeros(len(b), np.int32), colours(len(b), t), t
    yield "one box", [(37, 70)], np.array([(10, 8, 20, 12)], np.int32), np.zeros(1, np.int32), colours(1, 3), 5
    yield "five boxes", [(37, 70)], random_boxes(5, 37, 70, 5), np.zeros(5, np.int32), colours(5, 4), 2
    # many bands overlap: 300 boxes on 64 x 64 (every later box fits the workgroup's list), and 700, where the list of the early boxes
    # overflows and the rest are read from memory
    for k, t in ((300, 2), (300, 5)):
        yield f"{k} boxes t={t}", [(64, 64)], random_boxes(k, 64, 64, k + t), np.zeros(k, np.int32), colours(k, k), t
    for k, t in ((700, 1), (700, 5)):                       # large boxes from the top-left quarter: most strips meet most later boxes
        b = random_boxes(k, 28, 28, k + t, lo=30, hi=70)
        yield f"{k} boxes t={t}", [(64, 64)], b, np.zeros(k, np.int32), colours(k, k), t
    # two frames of different sizes in one call; frame indices out of range draw nothing
    b = np.concatenate([edge_boxes(37, 70), random_boxes(24, 50, 70, 9)])
    of = np.random.RandomState(3).randint(0, 2, size=len(b)).astype(np.int32)
    of[[1, 7, 20]] = (-1, 2, 1 << 30)
    yield "two frames", [(37, 70), (50, 23)], b, of, colours(len(b), 8), 5
    yield "two frames t=32", [(37, 70), (50, 23)], b, of, colours(len(b), 8), 32


def normalised_crops(b: int, seed: int):
    """Random uint8 crops through the builder's normalisation: (B,3,128,128) and (B,3,256,256) fp32, and the uint8 sources."""
    from feartracker_amd.train_data import _normalise_u8
    rng = np.random.RandomState(seed)
    t8 = rng.randint(0, 256, size=(b, 128, 128, 3)).astype(np.uint8)
    s8 = rng.randint(0, 256, size=(b, 256, 256, 3)).astype(np.uint8)
    return np.stack([_normalise_u8(x) for x in t8]), np.stack([_normalise_u8(x) for x in s8]), t8, s8


def miner_step(b: int, seed: int):
    """One step's worth of miner inputs: metricsgen's maps (pair 1 made invisible) and normalised crops; a few out-of-range and
    non-finite crop values, and on odd seeds a non-finite bbox cell at pair 0's arg-max."""
    import metricsgen as mg
    m = mg.step_maps(max(b, 5), seed)
    m = {k: np.ascontiguousarray(v[:b]) for k, v in m.items()}
    m["visible"][1] = 0                                     # an invisible pair among the rendered ones
    tmpl, srch, _, _ = normalised_crops(b, 100 + seed)
    srch[0, 0, 3, :5] = (np.nan, np.inf, -np.inf, 9.0, -9.0)
    tmpl[0, 2, 0, :3] = (7.5, -7.5, np.nan)
    if seed % 2:
        cell = int(np.argmax(m["cls"][0].reshape(-1)))
        m["bbox"].reshape(b, 4, -1)[0, :, cell] = (np.nan, np.inf, -3e9, 5.0)
    return dict(m, template=tmpl, search=srch)
