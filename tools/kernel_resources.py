#!/usr/bin/env python3
"""Register / scratch / occupancy table of every trace_kernel instantiation (hipcc -Rpass-analysis=kernel-resource-usage).
usage: python tools/kernel_resources.py [--unit NAME.hip ...] [extra hipcc flags]   (cross-compiles for gfx950, no GPU needed)
The instances live in rtw_launch.hip and, the BATCH && ACCUM ones, in rtw_batch_accum_f32.hip / _f64.hip: one table over all three.
--unit names other translation units instead (rtw_features.hip: the instances of the feature kernel, the batched ones among them; rtw_features_accum_batch_f32.hip /
_f64.hip: its tiled batched instances; rtw_denoise.hip: the denoiser's kernels and the batched level kernels; rtw_accum_kernels.hip: the accumulator's kernels, the noise map and the
batched resolve and noise map among them; rtw_temporal.hip: the instances of the temporal step, with and without moments, the temporal noise map and their batched (`paths`) twins; rtw_present.hip: the instances of the present kernel; rtw_motion.hip: the instances of the first-hit motion pass; rtw_rays.hip: the eight instances of the ray-query kernel (its LDS is dynamic: 11 KB + the scene copy, not in the table); rtw_trace_rays.hip: the eight instances of the radiance-query kernel (the same dynamic LDS); rtw_motion_blur.hip: the three kernels of the motion-blur stage; rtw_defocus.hip: the two kernels of the defocus stage (the gather's LDS is dynamic: (16 + 2*max_radius) * 192 elements, not in the table); rtw_wide_aperture.hip: the two kernels the wide-aperture stage adds, at both scales; both units: with their batched (`views`) twins; `motion`: the step instances that read its plane)."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = ""
units = []
while len(sys.argv) > 2 and sys.argv[1] == "--unit":
    units.append(sys.argv[2]); del sys.argv[1:3]
for unit in units or ("rtw_launch.hip", "rtw_batch_accum_f32.hip", "rtw_batch_accum_f64.hip"):
    src = os.path.join(ROOT, "raytracingweekend.jl_amd", "csrc", unit)
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", "/dev/null"] + sys.argv[1:]
    out += subprocess.run(cmd, capture_output=True, text=True).stderr
rows, cur = [], None
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}; rows.append(cur); continue
    m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
    if m and cur is not None:
        cur[m.group(1)] = int(m.group(2))
print(f"{'kernel':52s} {'VGPR':>5s} {'SGPR':>5s} {'waves':>5s} {'scratch B':>9s} {'vspill':>6s} {'sspill':>6s} {'LDS B':>6s}")
for r in rows:
    n = r["name"]
    m = re.match(r"_ZN3rtw12trace_kernelI([fd])Lb([01])ELb([01])ELb([01])ELb([01])ELi(n?\d+)ELb([01])ELb([01])ELb([01])E", n)
    if m:
        label = f"trace<{'f32' if m.group(1) == 'f' else 'f64'}{', profile' if m.group(2) == '1' else ''}{', lds-scene' if m.group(3) == '1' else ', global-scene'}{', cull' if m.group(4) == '1' else ''}{', mfma' if m.group(5) == '1' else ''}{', numerics fixed' if not m.group(6).startswith('n') else ''}{', batch' if m.group(7) == '1' else ''}{', accum' if m.group(8) == '1' else ''}{', adapt' if m.group(9) == '1' else ''}>"
    elif re.match(r"_ZN3rtw15features_kernelI([fd])Lb([01])ELb([01])ELi(n?\d+)E", n):
        m = re.match(r"_ZN3rtw15features_kernelI([fd])Lb([01])ELb([01])ELi(n?\d+)E(?:Lb([01])E)?(?:Lb([01])E)?", n)
        label = f"features<{'f32' if m.group(1) == 'f' else 'f64'}{', mfma' if m.group(2) == '1' else ', valu'}{', lds-scene' if m.group(3) == '1' else ', global-scene'}{', numerics fixed' if not m.group(4).startswith('n') else ''}{', tiled' if m.group(5) == '1' else ''}{', batch' if m.group(6) == '1' else ''}>"
    elif re.match(r"_ZN3rtw\d+dn_level_batchI([fd])", n):
        m = re.match(r"_ZN3rtw\d+dn_level_batchI([fd])(?:Lb([01])E)?", n)
        label = f"denoise level<{'f32' if m.group(1) == 'f' else 'f64'}{', guided' if m.group(2) == '1' else ''}, batch>"
    elif re.match(r"_ZN3rtw\d+dn_(prepare|level)I([fd])", n):
        m = re.match(r"_ZN3rtw\d+dn_(prepare|level)I([fd])(?:Lb([01])E)?", n)
        label = f"denoise {m.group(1)}<{'f32' if m.group(2) == 'f' else 'f64'}{', guided' if m.group(3) == '1' else ''}>"
    elif re.search(r"accum_(noise|resolve)_batch_kernelI([fd])", n):
        m = re.search(r"accum_(noise|resolve)_batch_kernelI([fd])", n)
        label = f"accum {m.group(1)}<{'f32' if m.group(2) == 'f' else 'f64'}, batch>"
    elif re.search(r"accum_resolve(_tiles)?_kernelI([fd])", n):
        m = re.search(r"accum_resolve(_tiles)?_kernelI([fd])", n)
        label = f"accum resolve<{'f32' if m.group(2) == 'f' else 'f64'}{', tiles' if m.group(1) else ''}>"
    elif re.search(r"accum_noise_kernelI([fd])", n):
        label = "accum noise<%s>" % ("f32" if re.search(r"accum_noise_kernelI([fd])", n).group(1) == "f" else "f64")
    elif re.match(r"_ZN3rtw\d+tp_stepI([fd])Lb([01])E", n):
        m = re.match(r"_ZN3rtw\d+tp_stepI([fd])Lb([01])E(?:Lb([01])E)?(?:Lb([01])E)?(?:Lb([01])E)?", n)
        label = f"temporal tp_step<{'f32' if m.group(1) == 'f' else 'f64'}{', has_prev' if m.group(2) == '1' else ', first frame'}{', moments' if m.group(3) == '1' else ''}{', paths' if m.group(4) == '1' else ''}{', motion' if m.group(5) == '1' else ''}>"
    elif re.match(r"_ZN3rtw\d+tp_step_clampedI([fd])Lb([01])ELb([01])E", n):
        m = re.match(r"_ZN3rtw\d+tp_step_clampedI([fd])Lb([01])ELb([01])E(?:Lb([01])E)?(?:Lb([01])E)?", n)
        label = f"temporal tp_step_clamped<{'f32' if m.group(1) == 'f' else 'f64'}{', moments' if m.group(2) == '1' else ''}{', guides' if m.group(3) == '1' else ''}{', paths' if m.group(4) == '1' else ''}{', motion' if m.group(5) == '1' else ''}>"
    elif re.match(r"_ZN3rtw\d+tp_noiseI([fd])", n):
        m = re.match(r"_ZN3rtw\d+tp_noiseI([fd])(?:Lb([01])E)?", n)
        label = f"temporal tp_noise<{'f32' if m.group(1) == 'f' else 'f64'}{', paths' if m.group(2) == '1' else ''}>"
    elif re.match(r"_ZN3rtw\d+pr_presentI([fd])Li([34])ELb([01])E", n):
        m = re.match(r"_ZN3rtw\d+pr_presentI([fd])Li([34])ELb([01])E", n)
        label = f"present pr_present<{'f32' if m.group(1) == 'f' else 'f64'}, C = {m.group(2)}{'' if m.group(2) == '4' else ', aligned rows' if m.group(3) == '1' else ', unaligned rows'}>"
    elif re.match(r"_ZN3rtw\d+motion_passI([fd])Lb([01])E", n):
        m = re.match(r"_ZN3rtw\d+motion_passI([fd])Lb([01])E", n)
        label = f"motion motion_pass<{'f32' if m.group(1) == 'f' else 'f64'}{', lds-scene' if m.group(2) == '1' else ', global-scene'}>"
    elif re.match(r"_ZN3rtw\d+mb_(velocity|neighbour)I([fd])E", n):
        m = re.match(r"_ZN3rtw\d+mb_(velocity|neighbour)I([fd])E", n)
        label = f"motion blur mb_{m.group(1)}<{'f32' if m.group(2) == 'f' else 'f64'}>"
    elif re.match(r"_ZN3rtw\d+mb_gatherI([fd])Lb([01])E", n):
        m = re.match(r"_ZN3rtw\d+mb_gatherI([fd])Lb([01])E", n)
        label = f"motion blur mb_gather<{'f32' if m.group(1) == 'f' else 'f64'}{', pass-through' if m.group(2) == '1' else ''}>"
    elif re.match(r"_ZN3rtw\d+df_(prepare|gather)I([fd])(?:Lb([01])E)?E", n):
        m = re.match(r"_ZN3rtw\d+df_(prepare|gather)I([fd])(?:Lb([01])E)?E", n)
        label = f"defocus df_{m.group(1)}<{'f32' if m.group(2) == 'f' else 'f64'}{', views' if m.group(3) == '1' else ''}>"
    elif re.match(r"_ZN3rtw\d+wa_(reduce|compose)I([fd])Li([24])E(?:Lb([01])E)?E", n):
        m = re.match(r"_ZN3rtw\d+wa_(reduce|compose)I([fd])Li([24])E(?:Lb([01])E)?E", n)
        label = f"wide aperture wa_{m.group(1)}<{'f32' if m.group(2) == 'f' else 'f64'}, {m.group(3)}{', views' if m.group(4) == '1' else ''}>"
    elif re.match(r"_ZN3rtw\d+cast_rays_kernelI([fd])Lb([01])ELb([01])E", n):
        m = re.match(r"_ZN3rtw\d+cast_rays_kernelI([fd])Lb([01])ELb([01])E", n)
        label = f"rays cast_rays<{'f32' if m.group(1) == 'f' else 'f64'}{', mfma' if m.group(2) == '1' else ', valu'}{', lds-scene' if m.group(3) == '1' else ', global-scene'}>"
    elif re.match(r"_ZN3rtw\d+trace_rays_kernelI([fd])Lb([01])ELb([01])E", n):
        m = re.match(r"_ZN3rtw\d+trace_rays_kernelI([fd])Lb([01])ELb([01])E", n)
        label = f"radiance trace_rays<{'f32' if m.group(1) == 'f' else 'f64'}{', mfma' if m.group(2) == '1' else ', valu'}{', lds-scene' if m.group(3) == '1' else ', global-scene'}>"
    elif "unit_kernel" in n:
        label = "unit_kernel<%s>" % ("f32" if "IfE" in n else "f64")
    else:
        label = n[:44]
    print(f"{label:52s} {r.get('VGPRs', 0):5d} {r.get('TotalSGPRs', 0):5d} {r.get('Occupancy [waves/SIMD]', 0):5d} {r.get('ScratchSize [bytes/lane]', 0):9d} {r.get('VGPRs Spill', 0):6d} {r.get('SGPRs Spill', 0):6d} {r.get('LDS Size [bytes/block]', 0):6d}")
