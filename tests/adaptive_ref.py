"""The definition of the per-tile error estimate and of the adaptive loop (include/rmr.h, DESIGN.md
§4.8), in numpy float32 with every operation rounded on its own, so that the GPU's tile errors and
sample counts can be compared bit for bit.

Tile (tx, ty) covers pixels [8 tx, 8 tx + 8) x [8 ty, 8 ty + 8); lane l is pixel (8 tx + (l & 7),
8 ty + (l >> 3)). A is the accumulator, B the half image (the running mean of the odd-indexed samples)."""
import numpy as np


def _lanes(img, fill):
    """(H, W, C) -> (TY, TX, 64, C) in lane order, pixels outside the image filled with `fill`."""
    H, W, C = img.shape
    TY, TX = (H + 7) // 8, (W + 7) // 8
    pad = np.full((TY * 8, TX * 8, C), fill, img.dtype)
    pad[:H, :W] = img
    return pad.reshape(TY, 8, TX, 8, C).transpose(0, 2, 1, 3, 4).reshape(TY, TX, 64, C)


def tile_error_ref(A, B, offset=1e-4):
    """The (TY, TX) float32 tile errors of the float32 images A, B (H, W, 4), vectorised."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    offset = np.float32(offset)
    H, W = A.shape[:2]
    inside = _lanes(np.ones((H, W, 1), bool), False)[..., 0]
    a, b = _lanes(A, 0), _lanes(B, 0)
    with np.errstate(all="ignore"):
        unsampled = inside & ((a[..., 3] == 0) | (b[..., 3] == 0))
        finite = np.isfinite(a[..., :3]).all(-1) & np.isfinite(b[..., :3]).all(-1)
        d = (np.abs(a[..., 0] - b[..., 0]) + np.abs(a[..., 1] - b[..., 1])) + np.abs(a[..., 2] - b[..., 2])
        s = (a[..., 0] + a[..., 1]) + a[..., 2]
        v = d / (offset + np.sqrt(np.maximum(s, np.float32(0))))
        v = np.where(inside & finite & ~unsampled, v, np.float32(0)).astype(np.float32)
        while v.shape[-1] > 1:
            v = v[..., 0::2] + v[..., 1::2]
        n_t = inside.sum(-1).astype(np.float32)
        e = (v[..., 0] / n_t).astype(np.float32)
    return np.where(unsampled.any(-1), np.float32(np.inf), e).astype(np.float32)


def tile_error_loop(A, B, offset=1e-4):
    """The same, literally: one pixel per lane, then the xor butterfly over steps 1 .. 32."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    offset = np.float32(offset)
    H, W = A.shape[:2]
    TY, TX = (H + 7) // 8, (W + 7) // 8
    out = np.zeros((TY, TX), np.float32)
    with np.errstate(all="ignore"):
        for ty in range(TY):
            for tx in range(TX):
                v = [np.float32(0)] * 64
                n_t, unsampled = 0, False
                for lane in range(64):
                    x, y = 8 * tx + (lane & 7), 8 * ty + (lane >> 3)
                    if x >= W or y >= H:
                        continue
                    n_t += 1
                    a, b = A[y, x], B[y, x]
                    if a[3] == 0 or b[3] == 0:
                        unsampled = True
                    elif np.isfinite(a[:3]).all() and np.isfinite(b[:3]).all():
                        d = (abs(a[0] - b[0]) + abs(a[1] - b[1])) + abs(a[2] - b[2])
                        s = (a[0] + a[1]) + a[2]
                        v[lane] = np.float32(d / (offset + np.sqrt(max(s, np.float32(0)))))
                for step in (1, 2, 4, 8, 16, 32):
                    v = [np.float32(v[lane] + v[lane ^ step]) for lane in range(64)]
                assert all(np.array_equal(v[0], q, equal_nan=True) for q in v)
                out[ty, tx] = np.float32(np.inf) if unsampled else np.float32(v[0] / np.float32(n_t))
    return out


def select_ref(err, block_tiles, threshold, open_blocks=None):
    """The decision rule: the blocks still open, as a (ceil(TY / bt), ceil(TX / bt)) bool array. A block's
    error is the maximum of its tiles' errors; an open block whose error is not > threshold closes."""
    err = np.asarray(err, np.float32)
    TY, TX = err.shape
    bt = int(block_tiles)
    BY, BX = -(-TY // bt), -(-TX // bt)
    pad = np.full((BY * bt, BX * bt), -np.inf, np.float32)
    pad[:TY, :TX] = np.where(np.isnan(err), -np.inf, err)
    block = pad.reshape(BY, bt, BX, bt).max(axis=(1, 3))
    above = block > np.float32(threshold)
    return above if open_blocks is None else (above & np.asarray(open_blocks, bool))


def tiles_of_blocks(open_blocks, TY, TX, block_tiles):
    """(TY, TX) bools: the tiles of the open blocks."""
    return np.repeat(np.repeat(open_blocks, block_tiles, 0), block_tiles, 1)[:TY, :TX]


def simulate(images, W, H, threshold, offset=1e-4, min_samples=16, pass_samples=16, max_samples=64, block_tiles=2):
    """The adaptive loop on the CPU. images(c) -> (A_c, B_c): the full-image accumulator and half image
    after c uniform samples (A_c = render(times[:c]), B_c = render(times[1:c:2])); a tile with count c has
    exactly those pixels, and its error depends on its own pixels alone. Returns a dict: counts (TY, TX)
    uint32, image (H, W, 4), passes, tiles_open, samples, max_error, errors (the tile errors at the stop)."""
    TY, TX = (H + 7) // 8, (W + 7) // 8
    cache = {}

    def at(c):
        if c not in cache:
            A, B = images(c)
            cache[c] = (A, tile_error_ref(A, B, offset))
        return cache[c]

    counts = np.full((TY, TX), min_samples, np.uint32)
    BY, BX = -(-TY // block_tiles), -(-TX // block_tiles)
    open_blocks = np.ones((BY, BX), bool)
    done, passes = min_samples, 1
    while True:
        err = np.zeros((TY, TX), np.float32)
        for c in np.unique(counts):
            err = np.where(counts == c, at(int(c))[1], err)
        open_blocks = select_ref(err, block_tiles, threshold, open_blocks)
        if not open_blocks.any() or done == max_samples:
            break
        n = min(pass_samples, max_samples - done)
        counts[tiles_of_blocks(open_blocks, TY, TX, block_tiles)] += n
        done += n
        passes += 1
    image = np.zeros((H, W, 4), np.float32)
    per_pixel = np.repeat(np.repeat(counts, 8, 0), 8, 1)[:H, :W]
    for c in np.unique(counts):
        m = per_pixel == c
        image[m] = at(int(c))[0][m]
    with np.errstate(invalid="ignore"):
        finite_max = np.float32(0)
        for e in err.ravel():
            if e > finite_max:
                finite_max = e
    return {"counts": counts, "image": image, "passes": passes,
            "tiles_open": int((err > np.float32(threshold)).sum()),
            "samples": int(per_pixel.astype(np.uint64).sum()), "max_error": np.float32(finite_max), "errors": err}


def oracle_images(orc, times):
    """images(c) for simulate() from an oracle.Oracle and the seeds: incremental renders, cached."""
    times = np.ascontiguousarray(times, np.float32)
    odd = np.ascontiguousarray(times[1::2])
    state = {"c": 0, "A": None, "B": None}
    memo = {}

    def images(c):
        if c in memo:
            return memo[c]
        assert c > state["c"], "counts are asked for in increasing order"
        c0 = state["c"]
        state["A"] = orc.render(times[c0:c], first_sample=c0, accum=None if state["A"] is None else state["A"].copy())
        h0, h1 = c0 // 2, c // 2
        if h1 > h0:
            state["B"] = orc.render(odd[h0:h1], first_sample=h0, accum=None if state["B"] is None else state["B"].copy())
        state["c"] = c
        B = state["B"] if state["B"] is not None else np.zeros_like(state["A"])
        memo[c] = (state["A"].copy(), B.copy())
        return memo[c]
    return images
