"""The witness of the first-hit feature buffers (include/rtw_hip.h rtw_render_features_*): the definition restated in Python from the
oracle's UNIT calls only -- rng_stream, rng_float, get_ray, hit_world, skycolor, fx_sum -- and the flat scene's own albedo.  Nothing of
the product is used.  It honours the oracle's current numerics mode (rtw_oracle.set_numerics / the `numerics` fixture of conftest.py).

    items(...)    every feature sample of a frame: the 8 binary64 values per (pixel, chunk) and what was hit
    resolve(...)  the 8 slots per pixel over a chunk range: exact sums (fx_sum), / chunk_count, rounded to T; NaN in all 8 when poisoned
Results are cached per (frame, precision, numerics mode): the tests share one computation and must leave it unchanged."""
import numpy as np

import rtw_oracle as O

CHANNELS = 8
_cache = {}


def effective_chunks(spp, n_chunks=0):
    """the default rule of rtw_params.n_chunks -> (N effective chunks, chunk size s)"""
    nch = int(n_chunks) if int(n_chunks) > 0 else min(int(spp), 256)
    nch = min(nch, int(spp))
    s = -(-int(spp) // nch)
    return -(-int(spp) // s), s


def frame_f(T):
    """the frame F of the feature tests: the random-spheres scene (485 spheres, all three materials) through a camera with a lens
    (aperture 0.1, so the disk sample matters), 32 x 18: the last tile row holds 2 pixel rows"""
    flat = O.scene_random_spheres(1, T)
    cam = O.default_camera([13, 2, 3], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.1, 10, T)
    return flat, cam, 32, 18


def _albedo(flat, idx, T):
    if int(flat["kind"][idx]) == 2:                  # Dielectric: scatter's attenuation is (1, 1, 1)
        return [1.0, 1.0, 1.0]
    return [float(np.dtype(T).type(flat[k][idx])) for k in ("ar", "ag", "ab")]


def items(flat, cam, W, H, spp, n_chunks, seed, T, key=None):
    """Every feature sample of the render: values float64 [H, W, N, 8], kind int [H, W, N] (the material kind hit, -1 on a miss).
    `key`: a name for (scene, camera) -- with it the result is cached (read-only)."""
    T = np.dtype(T).type
    ck = (key, W, H, spp, n_chunks, seed, np.dtype(T).name, O._default_numerics) if key is not None else None
    if ck in _cache:
        return _cache[ck]
    N, s = effective_chunks(spp, n_chunks)
    values = np.zeros((H, W, N, CHANNELS), np.float64)
    kind = np.full((H, W, N), -1, np.int32)
    w_div, h_div = T(np.float32(W)), T(np.float32(H))
    for j in range(1, W + 1):
        for i in range(1, H + 1):
            pix = (j - 1) * H + (i - 1)
            for c in range(N):
                st = O.rng_stream(seed, pix, c)
                du = dv = T(0)
                if c * s != 0:                                   # not sample 1 of the pixel: jittered (src/render.jl:30-31)
                    du = O.rng_float(st, T) / w_div
                    dv = O.rng_float(st, T) / h_div
                ray, st = O.get_ray(cam, T(j / W) + du, T((H - i) / H) + dv, st, T)
                idx, rec = O.hit_world(flat, ray[:3], ray[3:], 1e-4, np.inf, T)
                v = values[i - 1, j - 1, c]
                if idx >= 0:
                    v[0:3] = _albedo(flat, idx, T)
                    v[3:6] = rec[4:7]                            # HitRecord.n, face-forwarded
                    v[6] = rec[0]                                # HitRecord.t
                    v[7] = 1.0
                    kind[i - 1, j - 1, c] = int(flat["kind"][idx])
                else:
                    v[0:3] = O.skycolor(ray[3:], T)
    values.setflags(write=False)
    kind.setflags(write=False)
    out = dict(values=values, kind=kind, N=N, s=s)
    if ck is not None:
        _cache[ck] = out
    return out


def resolve(it, T, chunks=None):
    """-> (raw [H, W, 8] of dtype T, poisoned bool [H, W]) over the chunk range `chunks` = (begin, count) (None: all N)"""
    T = np.dtype(T).type
    begin, count = (0, it["N"]) if chunks is None else chunks
    vals = it["values"][:, :, begin:begin + count, :]
    H, W = vals.shape[:2]
    raw = np.zeros((H, W, CHANNELS), T)
    poisoned = np.zeros((H, W), bool)
    for i in range(H):
        for j in range(W):
            sums = [O.fx_sum(vals[i, j, :, k]) for k in range(CHANNELS)]
            if any(bad for _, bad in sums):
                poisoned[i, j] = True
                raw[i, j, :] = np.nan
            else:
                raw[i, j, :] = [T(sm / float(count)) for sm, _ in sums]
    return raw, poisoned


def coverage_census(it, chunks=None):
    """-> (pixels of coverage 0, pixels of fractional coverage, the set of material kinds hit) over a chunk range"""
    begin, count = (0, it["N"]) if chunks is None else chunks
    k = it["kind"][:, :, begin:begin + count]
    hits = (k >= 0).sum(axis=2)
    return int((hits == 0).sum()), int(((hits > 0) & (hits < count)).sum()), set(int(x) for x in np.unique(k[k >= 0]))


def bits(a):
    """the bit patterns of a float32 / float64 array"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
