"""The stderr lines of the stages' measurement aid (RTW_ENABLE_TEST_AIDS=1 with RTW_PRESENT_PROFILE, RTW_DENOISE_PROFILE and
RTW_TEMPORAL_PROFILE): every device-resident stage once in ONE fresh process (the variables are read once per process), and the lines it
leaves against the expressions the tools/gpu_*.py scripts parse them with.  Nothing is compared but the lines: their number per tag, their
fields, the precision, and that every time is a finite float >= 0.
The frame is 37 x 23 (the upsampler: 18 x 10 -> 37 x 23): the buffers are motion_blur_ref's hand-made case 1 of that size, the lens stages
look through a pinhole camera of the package, the motion pass sees test_gpu_motion's four spheres.  No stage refuses the frame."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, LO_W, LO_H = 37, 23, 18, 10
LEVELS = 2                          # of the upsampler

# tag -> [(who parses the line, the expression)]; a line of the tag must match one of them
PATTERNS = {
    # tools/gpu_present.py PR_LINE
    "rtw present": [r"^\[rtw present\] (f32|f64) (\d+)x(\d+) views=1 C=([34]) (dword|aligned|unaligned) ms=([0-9.]+)$"],
    # tools/gpu_upsample.py UP_LINE (it reads f32 alone; every upsampler call here is f32)
    "rtw upsample": [r"^\[rtw upsample\] f32 \S+ (prepare|level|upsample|total)(?: step=(\d+))?(?: levels=\d+)? ms=([0-9.]+)$"],
    # tools/gpu_defocus.py (re.match, no anchor behind the last field: anchored here)
    "rtw defocus": [r"^\[rtw defocus\] (f32|f64) (\d+)x(\d+) max_radius=\d+ prepare_ms=([\d.]+) gather_ms=([\d.]+)$"],
    # tools/gpu_wide_aperture.py: `pat`, built from its LAUNCHES (anchored here)
    "rtw wide_aperture": [r"^\[rtw wide_aperture\] (f32|f64) (\d+)x(\d+) max_radius=(\d+) " +
                          " ".join(k + r"_ms=([\d.]+)" for k in ("prepare", "gather", "wide_prepare", "reduce", "small_gather", "compose")) + "$"],
    # tools/gpu_motion_blur.py (anchored here)
    "rtw motion blur": [r"^\[rtw motion blur\] (f32|f64) (\d+)x(\d+) taps=\d+ velocity_ms=([\d.]+) neighbour_ms=([\d.]+) gather_ms=([\d.]+)$"],
    # no tool parses it by expression (tools/gpu_animation.py shows it): from launch_motion's format
    # "[rtw motion] %s %dx%d spheres=%d lds_scene=%d ms=%.5f\n"
    "rtw motion": [r"^\[rtw motion\] (f32|f64) (\d+)x(\d+) spheres=(\d+) lds_scene=([01]) ms=([0-9.]+)$"],
    "rtw temporal": [
        # tools/gpu_temporal.py TP_LINE
        r"^\[rtw temporal\] (f32|f64) (\d+)x(\d+) step prev=([01]) paths=0 ms=([0-9.]+)$",
        # tools/gpu_temporal_clamp.py CLAMP_LINE
        r"^\[rtw temporal\] (f32|f64) (\d+)x(\d+) (clamped|clamped\+moments) r=(\d) guides=(\d) paths=0 ms=([0-9.]+)$",
        # tools/gpu_temporal_noise.py NOISE_LINE
        r"^\[rtw temporal\] (f32|f64) (\d+)x(\d+) noise r=(\d) paths=0 ms=([0-9.]+)$"],
}
# the lines of the Float32 calls, per tag
COUNTS = {
    "rtw present": 1,
    "rtw upsample": LEVELS + 3,       # prepare, each level, upsample, total
    "rtw defocus": 2,                 # its own call, and the wide-aperture call with max_radius = 8
    "rtw wide_aperture": 1,
    "rtw motion blur": 1,
    "rtw motion": 1,
    "rtw temporal": 3,                # two steps and the noise map
}


def _child():
    """what the fresh process runs: every stage once on device buffers, Float32; the present stage once more in Float64"""
    import torch
    torch.cuda.init()
    import rtw_amd as rtw
    import motion_blur_ref as BR
    from test_gpu_motion import _four_spheres
    T = np.float32
    c = BR.handmade_blur_cases(H, W, T, BR.SEEDS[T])[1]
    lay = lambda a: np.array(np.swapaxes(a, 0, 1), order="C", copy=True)             # the library's layout: pixel (i, j) at j*H + i
    up = lambda a: torch.from_numpy(a).to("cuda:0")
    img, feat, mot = (up(lay(c[k])) for k in ("image", "features", "motion"))
    img_lo, feat_lo = (up(lay(c[k][::2, ::2][:LO_H, :LO_W])) for k in ("image", "features"))
    buf = lambda n_bytes: torch.zeros((int(n_bytes) + 3) // 4, dtype=torch.float32, device="cuda:0")
    out = buf(W * H * 3 * 4)
    cam, cam_prev = c["cam"], c["cam_prev"]
    lens_cam = rtw.default_camera(lookfrom=(3, 1, 2), lookat=(0, 0, -1), vup=(0, 1, 0), vfov=30, aspect_ratio=W / H, aperture=0, focus_dist=3.7, elem_type=T)
    say = lambda s: (torch.cuda.synchronize(), sys.stderr.flush(), print("[call] " + s, file=sys.stderr, flush=True))

    say("present")
    rtw.present_into(buf(rtw.present_bytes(W, H, 3)).data_ptr(), img.data_ptr(), W, H, elem_type=T)
    say("upsample")
    rtw.upsample_into(out.data_ptr(), img_lo.data_ptr(), feat_lo.data_ptr(), feat.data_ptr(), buf(rtw.upsample_work_bytes(LO_W, LO_H, T)).data_ptr(), LO_W, LO_H, W, H,
                      elem_type=T, levels=LEVELS)
    say("defocus")
    rtw.defocus_into(out.data_ptr(), buf(rtw.defocus_work_bytes(W, H, T)).data_ptr(), img.data_ptr(), feat.data_ptr(), lens_cam, W, H, elem_type=T, lens_radius=0.05, max_radius=8)
    for mr in (16, 8):
        say(f"wide_aperture {mr}")
        rtw.wide_aperture_into(out.data_ptr(), buf(rtw.wide_aperture_work_bytes(W, H, T, mr)).data_ptr(), img.data_ptr(), feat.data_ptr(), lens_cam, W, H, elem_type=T,
                               lens_radius=0.05, max_radius=mr)
    say("motion_blur")
    rtw.motion_blur_into(out.data_ptr(), buf(rtw.motion_blur_work_bytes(W, H, T)).data_ptr(), img.data_ptr(), feat.data_ptr(), mot.data_ptr(), cam, cam_prev, W, H, elem_type=T)
    say("first_hit_motion")
    renderer = rtw.DeviceRenderer(_four_spheres(rtw, T, 0.0)[0], cam, device=0)
    rtw.first_hit_motion_into(renderer, buf(W * H * 4 * 4).data_ptr(), W, H)
    say("temporal")
    st = [buf(rtw.temporal_state_bytes(W, H, T)) for _ in range(2)]
    rtw.temporal_step_into(out.data_ptr(), st[0].data_ptr(), img.data_ptr(), feat.data_ptr(), cam_prev, W, H, elem_type=T)
    rtw.temporal_step_clamped_into(out.data_ptr(), st[1].data_ptr(), img.data_ptr(), feat.data_ptr(), cam, W, H, d_state_prev_ptr=st[0].data_ptr(), cam_prev=cam_prev, elem_type=T)
    say("temporal_noise")
    rtw.temporal_noise_into(out.data_ptr(), st[1].data_ptr(), buf(rtw.temporal_moment_bytes(W, H, T)).data_ptr(), W, H, elem_type=T)
    say("present f64")
    img64 = up(lay(c["image"]).astype(np.float64))
    rtw.present_into(buf(rtw.present_bytes(W, H, 4, 0)).data_ptr(), img64.data_ptr(), W, H, elem_type=np.float64, channels=4)
    torch.cuda.synchronize()
    print("ran")


def test_every_stage_leaves_the_lines_the_tools_parse():
    """one fresh process with the master switch and the three profile variables set; the counts of COUNTS for Float32, one present line for Float64"""
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    code = "import sys\nsys.path[:0] = [%r, %r, %r]\nimport test_gpu_stage_aids as S\nS._child()\n" % (tests, root, os.path.join(root, "oracle"))
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DENOISE_PROFILE="1", RTW_TEMPORAL_PROFILE="1", RTW_PRESENT_PROFILE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    print(r.stderr[-6000:])
    assert r.returncode == 0 and "ran" in r.stdout, r.stderr[-3000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[rtw ")]
    by_tag = {tag: [] for tag in PATTERNS}
    for ln in lines:
        tag = ln[1:ln.index("]")]
        assert tag in PATTERNS, ln                                  # (no denoiser line: the upsampler prints its own)
        assert any(re.match(p, ln) for p in PATTERNS[tag]), ln
        by_tag[tag].append(ln)
        # every time is a finite float >= 0, written with five decimals
        times = re.findall(r"ms=(\S+)", ln)
        assert times, ln
        for t in times:
            assert re.fullmatch(r"\d+\.\d{5}", t) and math.isfinite(float(t)) and float(t) >= 0, ln
    f32 = {tag: [ln for ln in ls if ln.split()[len(tag.split())] == "f32"] for tag, ls in by_tag.items()}
    f64 = [ln for ln in lines if " f64 " in ln]
    assert {tag: len(ls) for tag, ls in f32.items()} == COUNTS, by_tag
    assert len(lines) == sum(COUNTS.values()) + 1 and f64 == by_tag["rtw present"][1:], lines
    assert f" f32 {W}x{H} views=1 C=3 unaligned ms=" in by_tag["rtw present"][0] and f" f64 {W}x{H} views=1 C=4 dword ms=" in f64[0]
    size = f" f32 {LO_W}x{LO_H}->{W}x{H} "
    kinds = [ln.split(size)[1].split(" ms=")[0] for ln in by_tag["rtw upsample"]]
    assert kinds == ["prepare"] + [f"level step={1 << k}" for k in range(LEVELS)] + ["upsample", f"total levels={LEVELS}"], by_tag["rtw upsample"]
    assert all(f" f32 {W}x{H} max_radius=8 prepare_ms=" in ln for ln in by_tag["rtw defocus"])          # (one view: no n_views field)
    assert f" f32 {W}x{H} max_radius=16 prepare_ms=" in by_tag["rtw wide_aperture"][0] and len(re.findall(r"_ms=", by_tag["rtw wide_aperture"][0])) == 6
    assert f" f32 {W}x{H} taps=15 velocity_ms=" in by_tag["rtw motion blur"][0] and len(re.findall(r"_ms=", by_tag["rtw motion blur"][0])) == 3
    assert f" f32 {W}x{H} spheres=4 lds_scene=" in by_tag["rtw motion"][0]
    tp = [ln.split(f" f32 {W}x{H} ")[1].split(" ms=")[0] for ln in by_tag["rtw temporal"]]
    assert tp == ["step prev=0 paths=0", "clamped r=1 guides=0 paths=0", "noise r=2 paths=0"], by_tag["rtw temporal"]
    # the order of the lines is the order of the calls
    order = [ln[1:ln.index("]")] for ln in lines]
    assert order == ["rtw present"] + ["rtw upsample"] * (LEVELS + 3) + ["rtw defocus", "rtw wide_aperture", "rtw defocus", "rtw motion blur", "rtw motion"] + ["rtw temporal"] * 3 + \
        ["rtw present"], order
