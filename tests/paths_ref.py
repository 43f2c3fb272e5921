"""The witness of the batched temporal steps (include/rtw_hip.h rtw_reproject_*, rtw_render_paths_*).  A batched step has NO arithmetic of its
own: path s of a batch is the single step of path s.  So the witness is the single witnesses (temporal_ref, temporal_noise_ref,
temporal_clamp_ref) side by side, plus the packers of the strided layouts the batched entry points read and write.

    path_inputs(H, W, T, s, n_frames)        the hand-made inputs of path s: cameras, frames, a previous state, its moment plane, its camera
    step(inputs, k, T, prev, ...)            the witness of step k of every path: the single witnesses, one call per path
    table(cams, cams_prev, T)                the table of rtw_reproject_table_* restated from temporal_ref.host_constants and the camera fields
    pack_* / unpack_*                        lists of per-path arrays <-> the library's memory (paths one behind the other, at their strides)
Arrays are indexed [i, j, channel] like the single witnesses'."""
import numpy as np

import temporal_clamp_ref as CR
import temporal_noise_ref as NR
import temporal_ref as TR

#: path s of the tests: temporal_ref.PATH with lookfrom and lookat shifted by s times these, so that the paths differ in every table element
FROM_SHIFT, AT_SHIFT = (0.05, -0.04, 0.03), (0.1, 0.05, 0.0)
N_PATHS = 3
#: the clamp of the tests (guides on for odd s is a property of the CENSUS only: one launch shares one clamp)
CLAMP = dict(radius=1, guides=False, sigma=1.0, len_scale=0.5)


def _shift(p, d, s):
    return tuple(float(a) + s * float(b) for a, b in zip(p, d))


def path_cameras(T, s, W, H, n_frames=3, rtw=None):
    """-> (cams, cam0): the cameras of path s along the shifted PATH and the camera of its hand-made previous state, shifted alike"""
    if rtw is None:
        import rtw_amd as rtw
    cams = [TR.make_camera(rtw, T, _shift(f, FROM_SHIFT, s), _shift(a, AT_SHIFT, s), W, H) for f, a in TR.PATH[:n_frames]]
    cam0 = TR.make_camera(rtw, T, _shift((-0.1, -0.05, 0.02), FROM_SHIFT, s), _shift((-0.3, 0.1, -1.0), AT_SHIFT, s), W, H)
    return cams, cam0


def path_inputs(H, W, T, s, n_frames=3, rtw=None):
    """-> (cams, frames, state0, moment0, cam0) of path s: temporal_noise_ref.handmade_sequence on the seed SEEDS[T] + 100 s of temporal_ref
    (its frames, previous state and moment plane) seen through the path's own cameras"""
    T = np.dtype(T).type
    _, frames, state0, moment0, _ = NR.handmade_sequence(H, W, T, TR.SEEDS[T] + 100 * s, n_frames, rtw)
    cams, cam0 = path_cameras(T, s, W, H, n_frames, rtw)
    return cams, frames, state0, moment0, cam0


def step(inputs, k, T, prev, moments=False, clamp=None, **kw):
    """step k of every path.  inputs: a list of path_inputs; prev: None (first frames) or a list of (state, moment or None, cam_prev) per path
    -> a list of (out, next state, next moment plane or None) per path: the single witness of the form, called once per path"""
    res = []
    for s, (cams, frames, _, _, _) in enumerate(inputs):
        st, mo, cp = prev[s] if prev is not None else (None, None, None)
        if clamp is not None:
            res.append(CR.step_clamped(*frames[k], cams[k], T, st, cp, mo if moments else None, moments=moments, clamp=clamp, **kw))
        elif moments:
            res.append(NR.step_moments(*frames[k], cams[k], T, st, mo, cp, **kw))
        else:
            res.append(TR.step(*frames[k], cams[k], T, st, cp, **kw) + (None,))
    return res


def table(cams, cams_prev, T):
    """the (n_paths, 32) table of the header, restated: the camera fields as they are, the projection's constants from temporal_ref.host_constants"""
    T = np.dtype(T).type
    tab = np.zeros((len(cams), 32), T)
    for s, cam in enumerate(cams):
        for k, name in enumerate(("origin", "lower_left_corner", "horizontal", "vertical")):
            tab[s, 3 * k:3 * k + 3] = np.asarray(getattr(cam, name), dtype=T)
        if cams_prev is not None:
            cp = cams_prev[s]
            for k, name in enumerate(("origin", "w", "horizontal", "vertical")):
                tab[s, 12 + 3 * k:15 + 3 * k] = np.asarray(getattr(cp, name), dtype=T)
            K = TR.host_constants(cp, T, 0.1, 0.25, 16.0)
            tab[s, 24:29] = [K[n] for n in ("Kw", "Qh", "Qv", "ih", "iv")]
    return tab


def pack_frames(arrays):
    """a list of [H, W, C] (or [H, W]) arrays -> the paths one behind the other, each pixel (i, j) at j*H + i"""
    return np.concatenate([np.ascontiguousarray(np.swapaxes(a, 0, 1)).reshape(-1) for a in arrays])


def unpack_frames(flat, n_paths, H, W, C=None):
    shape = (W, H) if C is None else (W, H, C)
    return [np.swapaxes(a.reshape(shape), 0, 1).copy() for a in np.asarray(flat).reshape(n_paths, -1)]


def pack_states(states, T, fill=0.0):
    """a list of states -> the packed states one behind the other at the stride of rtw_temporal_state_bytes; the padding holds `fill`"""
    H, W = states[0]["L"].shape
    flat = np.full((len(states), TR.state_elems(H, W, T)), fill, T)
    for s, st in enumerate(states):
        flat[s, :9 * W * H] = TR.pack_state(st, T)[:9 * W * H]
    return flat.reshape(-1)


def unpack_states(flat, n_paths, H, W):
    return [TR.unpack_state(a, H, W) for a in np.asarray(flat).reshape(n_paths, -1)]


def pack_moments(moments, T, fill=0.0):
    H, W = moments[0].shape
    flat = np.full((len(moments), NR.moment_elems(H, W, T)), fill, T)
    for s, mo in enumerate(moments):
        flat[s, :W * H] = NR.pack_moment(mo, T)[:W * H]
    return flat.reshape(-1)


def unpack_moments(flat, n_paths, H, W):
    return [NR.unpack_moment(a, H, W) for a in np.asarray(flat).reshape(n_paths, -1)]


def state_padding(flat, n_paths, H, W):
    """the padding elements between packed states (none when the state's bytes are a multiple of 16)"""
    return np.asarray(flat).reshape(n_paths, -1)[:, 9 * W * H:]


def moment_padding(flat, n_paths, H, W):
    return np.asarray(flat).reshape(n_paths, -1)[:, W * H:]
