"""The inputs of tests/test_gpu_filter_batch.py can tell a wrong batched filter from a right one (CPU only; the witness is
tests/denoise_ref.py, nothing of the product's arithmetic runs here).  A batch lies in memory exactly like ONE frame N*W wide, so the
wrong kernel to fear is the one that bounds its taps by that glued frame.  On every filter test frame:
  * the witness applied per view differs from the witness of the glued frame in every view that has a neighbour -- except a view whose
    every pixel is invalid (the NaN view of the 1 x 1 frames: NaN either way, nothing to compare);
  * the NaN pixel on a view's border column changes the neighbouring view's result in the glued frame, and none of its per-view results.
The Python names of the feature exist (they are what the GPU tests call)."""
import numpy as np
import pytest

import denoise_ref as DR
import filter_batch_frames as FB


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("N,W,H,levels", FB.FILTER_FRAMES)
def test_per_view_and_glued_witness_differ_in_every_view(N, W, H, levels, T):
    per_view = FB.witness(N, W, H, T, levels, 1, True, 1)
    glued = FB.witness_glued(N, W, H, T, levels)
    assert per_view.shape == glued.shape == (N, H, W, 3)
    for v in range(N):
        if np.isnan(per_view[v]).all():
            assert (W, H) == (1, 1) and v == FB.NAN_VIEW
            continue
        assert not DR.same_bits(per_view[v], glued[v]), f"view {v} of {N} x {W}x{H}: a filter that crosses the views' borders would go unseen"


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("N,W,H,levels", FB.FILTER_FRAMES)
def test_the_nan_pixel_reaches_the_neighbour_only_in_the_glued_frame(N, W, H, levels, T):
    i, j = FB.nan_pixel(W, H)
    images, _ = FB.views(N, W, H, T)
    assert j == W - 1 and np.isnan(images[FB.NAN_VIEW, i, j]).any()
    clean_images, _ = FB.views(N, W, H, T, with_nan=False)
    assert np.isfinite(clean_images[FB.NAN_VIEW, i, j]).all()
    nb = FB.NAN_VIEW + 1
    glued, glued_clean = FB.witness_glued(N, W, H, T, levels), FB.witness_glued(N, W, H, T, levels, with_nan=False)
    assert not DR.same_bits(glued[nb], glued_clean[nb]), "the NaN pixel does not reach the neighbouring view even in the glued frame"
    per_view, per_view_clean = FB.witness(N, W, H, T, levels, 1, True, 1), FB.witness(N, W, H, T, levels, 1, True, 1, with_nan=False)
    for v in range(N):
        if v != FB.NAN_VIEW:
            assert DR.same_bits(per_view[v], per_view_clean[v]), v
    assert np.isnan(per_view[FB.NAN_VIEW, i, j]).all() and not DR.same_bits(per_view[FB.NAN_VIEW], per_view_clean[FB.NAN_VIEW])


def test_the_stacking_helpers_are_the_librarys_layout():
    N, W, H = 3, 5, 3
    a = np.arange(N * H * W * 2, dtype=np.float32).reshape(N, H, W, 2)
    assert np.array_equal(FB.unglue(FB.glue(a), N), a)
    # the batch's memory is the glued frame's memory: view v, column j, row i at (v*W + j)*H + i
    assert np.array_equal(FB.lib_layout(a).reshape(-1), np.ascontiguousarray(FB.glue(a).transpose(1, 0, 2)).reshape(-1))


def test_python_names_exist(rtw):
    for name in ("render_features_batch", "features_batch_into", "denoise_batch", "denoise_batch_into", "render_denoised_batch"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert callable(rtw.DeviceRenderer.features_batch_into)
