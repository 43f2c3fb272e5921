"""The inputs of the batched filter tests (include/rtw_hip.h rtw_filter_batch_*): views stacked the way the library holds a batch.  No new
arithmetic: the witness stays tests/denoise_ref.py, applied view by view.

A batch of N frames of W x H lies in memory as view v, column j, row i at (v*W + j)*H + i -- which is also ONE frame of width N*W, the
views glued side by side (`glue`).  A kernel that bounded its taps by the batch instead of by each view would compute the witness of that
glued frame; tests/test_filter_batch_ref.py shows that the two differ on these very inputs."""
import functools

import numpy as np

import denoise_ref as DR

#: (views, W, H, levels): 1 x 1 frames; 5 x 3 with step 4 (taps at +-8 rows and columns lie beyond the whole frame, so inside the neighbouring
#: views of the glued frame); 851 pixels per view (a 256-lane block straddles views); several blocks per view with five levels
FILTER_FRAMES = [(4, 1, 1, 3), (5, 5, 3, 3), (3, 37, 23, 3), (2, 70, 41, 5)]
# (view v: SEED + 100 v.  A seed is usable when the 1 x 1 views -- one pixel each -- see each other in the glued frame at all, i.e. their
#  coverages do not cancel the weight; tests/test_filter_batch_ref.py is the check of that choice, in both precisions)
SEED = 31
NAN_VIEW = 0        # this view carries a NaN in its last column, next to view 1


def nan_pixel(W, H):
    """(row, column) of the NaN pixel of view NAN_VIEW: on the border column next to the following view"""
    return H // 2, W - 1


@functools.lru_cache(maxsize=None)
def views(N, W, H, T, with_nan=True):
    """-> (images [N, H, W, 3], features [N, H, W, 8]), read-only: denoise_ref.handmade frames, a different seed per view"""
    pairs = [DR.handmade(H, W, T, SEED + 100 * v) for v in range(N)]
    images, feats = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    i, j = nan_pixel(W, H)
    if with_nan:
        images[NAN_VIEW, i, j, 1] = np.nan
    else:                                        # (the same pixel, finite whatever handmade put there)
        images[NAN_VIEW, i, j, :] = 0.5
        feats[NAN_VIEW, i, j, :] = np.array([0.5, 0.5, 0.5, 0.0, 0.0, 1.0, 2.0, 1.0], T)
    images.setflags(write=False)
    feats.setflags(write=False)
    return images, feats


def glue(a):
    """[N, H, W, c] -> [H, N*W, c]: the views side by side as ONE frame"""
    return np.concatenate(list(a), axis=1)


def unglue(a, N):
    """[H, N*W, c] -> [N, H, W, c]"""
    return np.stack(np.split(a, N, axis=1))


def lib_layout(a):
    """[N, H, W, c] -> the library's memory: view v, pixel (i, j) at (v*W + j)*H + i"""
    return np.array(a.transpose(0, 2, 1, 3), order="C", copy=True)


@functools.lru_cache(maxsize=None)
def witness(N, W, H, T, levels, m, demodulate, gamma, with_nan=True):
    """the single-frame witness applied view by view -> [N, H, W, 3], read-only"""
    images, feats = views(N, W, H, T, with_nan)
    out = np.stack([DR.denoise(images[v], feats[v], T, levels=levels, m=m, demodulate=demodulate, gamma=gamma) for v in range(N)])
    out.setflags(write=False)
    return out


def witness_glued(N, W, H, T, levels, with_nan=True):
    """what a filter that ignored the views' borders would give: the witness of the glued frame, cut back into views"""
    images, feats = views(N, W, H, T, with_nan)
    return unglue(DR.denoise(glue(images), glue(feats), T, levels=levels), N)
