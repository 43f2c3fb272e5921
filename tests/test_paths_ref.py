"""CPU: the witness of the batched temporal steps (tests/paths_ref.py) and the inputs of tests/test_gpu_paths.py.  The witness has no arithmetic
of its own, so what is checked here is (1) that its packers are inverse to each other and leave the padding alone, and (2) that the per-path
hand-made inputs reach the regimes in which a batched kernel could go wrong -- above all taps that cross the frame's edge, where a kernel
that did not bound its taps by W and H would read the neighbouring path.  The conditions are `>= 1` on the existing census functions: no GPU
comparison can pass on inputs that never reach the edge."""
import numpy as np
import pytest

import paths_ref as PR
import temporal_clamp_ref as CR
import temporal_noise_ref as NR
import temporal_ref as TR

TYPES = [np.float32, np.float64]


def _chain(inputs, T, moments, clamp_of):
    """three chained steps of every path from its hand-made previous state -> per (path, step): (frame, cam, state, moment, cam_prev)"""
    prev = [(st, mo, c0) for (_, _, st, mo, c0) in inputs]
    for k in range(3):
        yield k, prev
        res = [PR.step([inp], k, T, [prev[s]], moments=moments, clamp=clamp_of(s))[0] for s, inp in enumerate(inputs)]
        prev = [(r[1], r[2], inputs[s][0][k]) for s, r in enumerate(res)]


@pytest.mark.parametrize("T", TYPES)
def test_the_plain_inputs_reach_the_frame_edge(T):
    W, H = 3, 2
    inputs = [PR.path_inputs(H, W, T, s) for s in range(PR.N_PATHS)]
    for k, prev in _chain(inputs, T, False, lambda s: None):
        for s, (cams, frames, _, _, _) in enumerate(inputs):
            c = TR.census(*frames[k], cams[k], T, prev[s][0], prev[s][2])
            resets = c["reset_not_front"] + c["reset_not_inr"] + c["reset_low_weight"]
            what = f"{np.dtype(T).name} path {s} step {k}: {c}"
            assert c["accepted"] >= 1 and c["fewer_than_4_inside"] >= 1 and resets >= 1, what


@pytest.mark.parametrize("size", [(37, 23), (70, 40)])
@pytest.mark.parametrize("T", TYPES)
def test_the_clamped_and_noise_inputs_reach_their_regimes(T, size):
    W, H = size
    inputs = [PR.path_inputs(H, W, T, s) for s in range(PR.N_PATHS)]
    clamp_of = lambda s: dict(PR.CLAMP, guides=bool(s & 1))
    for k, prev in _chain(inputs, T, True, clamp_of):
        for s, (cams, frames, _, _, _) in enumerate(inputs):
            st, mo, cp = prev[s]
            c = CR.census(*frames[k], cams[k], T, st, cp, mo, clamp=clamp_of(s))
            what = f"{np.dtype(T).name} {size} path {s} step {k}: {c}"
            for key in ("clamped_lo", "clamped_hi", "untouched", "len_shortened"):
                assert c[key] >= 1, (key, what)
            assert c["cut_top"] + c["cut_bottom"] >= 1 and c["cut_left"] + c["cut_right"] >= 1, what
            n = NR.census(*frames[k], cams[k], T, st, mo, cp)
            assert n["temporal"] >= 1 and n["spatial"] >= 1, f"{np.dtype(T).name} {size} path {s} step {k}: {n}"


@pytest.mark.parametrize("T", TYPES)
def test_the_paths_differ_in_every_camera_element_of_the_table(T):
    W, H = 37, 23
    cams = [PR.path_cameras(T, s, W, H) for s in range(PR.N_PATHS)]
    tab = PR.table([c[0][1] for c in cams], [c[0][0] for c in cams], T)
    assert tab.shape == (PR.N_PATHS, 32) and not tab[:, 29:].any()
    for a in range(PR.N_PATHS):
        for b in range(a + 1, PR.N_PATHS):
            same = [k for k in range(29) if TR.bits(tab[a, k:k + 1]) == TR.bits(tab[b, k:k + 1])]
            # (what may coincide: horizontal has no y component under vup = (0, 1, 0), in the current and the previous camera; Kw .. iv depend
            # on the viewport's size and the focus distance alone, which the paths share, so they differ by rounding at the most)
            assert set(same) <= {7, 19, 24, 25, 26, 27, 28}, (a, b, same)
    first = PR.table([c[0][0] for c in cams], None, T)
    assert not first[:, 12:].any() and TR.same_bits(first[:, :12], PR.table([c[0][0] for c in cams], [c[1] for c in cams], T)[:, :12])


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 23)])
@pytest.mark.parametrize("T", TYPES)
def test_the_packers_are_inverse_and_leave_the_padding(T, size):
    W, H = size
    inputs = [PR.path_inputs(H, W, T, s) for s in range(PR.N_PATHS)]
    states, moments = [i[2] for i in inputs], [i[3] for i in inputs]
    fs, fm = PR.pack_states(states, T, fill=-7.0), PR.pack_moments(moments, T, fill=-7.0)
    eb = np.dtype(T).itemsize
    assert fs.size * eb == PR.N_PATHS * ((9 * W * H * eb + 15) // 16 * 16) and fm.size * eb == PR.N_PATHS * ((W * H * eb + 15) // 16 * 16)
    for got, ref in zip(PR.unpack_states(fs, PR.N_PATHS, H, W), states):
        assert TR.same_state(got, ref)
    for got, ref in zip(PR.unpack_moments(fm, PR.N_PATHS, H, W), moments):
        assert TR.same_bits(got, ref)
    assert (PR.state_padding(fs, PR.N_PATHS, H, W) == -7.0).all() and (PR.moment_padding(fm, PR.N_PATHS, H, W) == -7.0).all()
    if (W * H) % 2:                                                # an odd frame leaves padding behind every state and plane
        assert PR.state_padding(fs, PR.N_PATHS, H, W).size > 0 and PR.moment_padding(fm, PR.N_PATHS, H, W).size > 0
    # path s of the packed states is the single packer's state at the stride of rtw_temporal_state_bytes
    n = TR.state_elems(H, W, T)
    for s, st in enumerate(states):
        assert TR.same_bits(fs[s * n:s * n + 9 * W * H], TR.pack_state(st, T)[:9 * W * H])
    frames = [i[1][0][0] for i in inputs]
    for got, ref in zip(PR.unpack_frames(PR.pack_frames(frames), PR.N_PATHS, H, W, 3), frames):
        assert TR.same_bits(got, ref)


@pytest.mark.parametrize("T", TYPES)
def test_the_witness_is_the_single_witnesses_side_by_side(T):
    W, H = 5, 3
    inputs = [PR.path_inputs(H, W, T, s) for s in range(PR.N_PATHS)]
    prev = [(st, mo, c0) for (_, _, st, mo, c0) in inputs]
    res = PR.step(inputs, 0, T, prev, moments=True, clamp=PR.CLAMP)
    for s, (cams, frames, st, mo, c0) in enumerate(inputs):
        assert CR.same_step(res[s], CR.step_clamped(*frames[0], cams[0], T, st, c0, mo, clamp=PR.CLAMP))
    res = PR.step(inputs, 0, T, None)
    for s, (cams, frames, _, _, _) in enumerate(inputs):
        ref = TR.step(*frames[0], cams[0], T)
        assert TR.same_bits(res[s][0], ref[0]) and TR.same_state(res[s][1], ref[1]) and res[s][2] is None
