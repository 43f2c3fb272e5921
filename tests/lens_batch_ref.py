"""The batched lens stages (include/rtw_hip.h rtw_lens_table_*, rtw_lens_batch_*) restated for the tests: the lens table from the witnesses'
own pieces, and batches of views built from the wide-aperture witness's hand-made cases.  There is no new arithmetic to restate: view v of a
batch IS wide_aperture_ref.wide_aperture of view v, and that is what the tests compare against."""
import numpy as np

import defocus_ref as FO
import paths_ref as PA
import wide_aperture_ref as WA

#: the frames of the GPU tests (W, H), from defocus_ref.SIZES: one pixel; partial tiles and partial blocks in both directions; a one-pixel
#: last small tile at both scales (130 / 2 = 65 and 130 / 4 = 33 small pixels)
SIZES = [(1, 1), (17, 33), (33, 17), (130, 5)]
RADII = [8, 16, 32]
#: the hand-made cases a batch's views are taken from (wide_aperture_ref.CASE_PARAMS): K = 40 px with a focus override of 6, K = 6 px and
#: K = 10 px at the camera's own focus -- three different (lens_radius, focus_dist) pairs
VIEW_CASES = (5, 8, 10)
#: the views' cameras: the case's own, then two that look from elsewhere at another focus distance (so F and every ray differ per view)
VIEW_CAMERAS = (None, dict(focus=5.0, origin=(-1.0, 0.5, 2.0)), dict(focus=3.0, origin=(0.25, 0.0, -1.5)))


def lens_table(cams, T, W, lens_radii, focus_dists):
    """the (n_views, 32) table of the header, restated: elements 0..28 the reprojection table's entry of each camera as its own previous
    one, 29 and 30 the defocus stage's host constants F and K, 31 zero"""
    T = np.dtype(T).type
    tab = PA.table(cams, cams, T)
    assert tab.shape == (len(cams), 32) and not tab[:, 29:].any()
    for v, cam in enumerate(cams):
        F, K, _ = FO.host_constants(cam, T, W, lens_radii[v], focus_dists[v], 8)
        tab[v, 29], tab[v, 30] = F, K
    return tab


def views(H, W, T):
    """three views of one frame size, each with its own image, features, camera and lens -> list of dicts image, features, cam, lens_radius,
    focus_dist (read-only arrays)"""
    T = np.dtype(T).type
    cases = WA.handmade_cases(H, W, T, WA.SEEDS[T])
    out = []
    for n, kw in zip(VIEW_CASES, VIEW_CAMERAS):
        c = cases[n]
        cam = c["cam"] if kw is None else FO.handmade_camera(H, W, T, **kw)
        for a in (c["image"], c["features"]):
            a.setflags(write=False)
        out.append(dict(image=c["image"], features=c["features"], cam=cam, lens_radius=c["params"]["lens_radius"], focus_dist=c["params"]["focus_dist"]))
    assert len({(v["lens_radius"], v["focus_dist"]) for v in out}) == 3 and sum(v["focus_dist"] > 0 for v in out) == 1
    return out


def witness(view, T, max_radius, gamma, frame=None):
    """wide_aperture_ref.wide_aperture of one view (on the frame of `frame`, another view, when given: the bracket) -> (out, the work dict)"""
    src = view if frame is None else frame
    out, work = WA.wide_aperture(src["image"], src["features"], view["cam"], T, view["lens_radius"], view["focus_dist"], max_radius, gamma)
    for a in (out, *work.values()):
        a.setflags(write=False)
    return out, work


def as_camera(cam, T):
    """a witness camera (defocus_ref.Cam) as the package's Camera, field for field: what its Python layer takes"""
    from rtw_amd.structs import Camera
    T = np.dtype(T).type
    return Camera(**{k: np.asarray(getattr(cam, k), dtype=T) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")}, lens_radius=T(cam.lens_radius))
