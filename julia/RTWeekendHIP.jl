# RTWeekendHIP.jl -- the reference-side binding a maintainer of claforte/RayTracingWeekend.jl
# would add to route `render` through librtw_hip.so (C ABI: include/rtw_hip.h).
#
# NOT EXECUTED in this repository's CI: the build image has no `julia`.  It is kept small on
# purpose -- everything testable lives behind the C ABI (tests/ call exactly these entry points
# through ctypes).  See INTEGRATION.md.
#
# Usage (inside the reference package, after `include("RTWeekendHIP.jl")`):
#     using .RTWeekendHIP
#     img = RTWeekendHIP.render(scene_random_spheres(elem_type=Float32), t_cam1, 1920, 1000)
# Same positional signature and return type as RayTracingWeekend.render (src/render.jl:8-44):
# Matrix{RGB{T}} of size (image_width ÷ 16//9, image_width), gamma-2 applied, unclamped.
module RTWeekendHIP

using Images: RGB
using StaticArrays
using ..RayTracingWeekend: Sphere, Lambertian, Metal, Dielectric, Camera, HittableList, Hittable

const LIB = get(ENV, "RTW_HIP_LIB", joinpath(@__DIR__, "..", "raytracingweekend.jl_amd", "lib", "librtw_hip.so"))

# rtw_scene_f32 / rtw_scene_f64 (include/rtw_hip.h): SoA view of a HittableList of Sphere{T}
struct CScene{T}
    n::Int32
    cx::Ptr{T}; cy::Ptr{T}; cz::Ptr{T}; r::Ptr{T}
    kind::Ptr{Int32}
    ar::Ptr{T}; ag::Ptr{T}; ab::Ptr{T}
    param::Ptr{T}
end

# rtw_camera_*: the 22 scalars of Camera{T} in the field order of src/camera.jl:2-9
struct CCamera{T}
    origin::NTuple{3,T}; lower_left_corner::NTuple{3,T}; horizontal::NTuple{3,T}; vertical::NTuple{3,T}
    u::NTuple{3,T}; v::NTuple{3,T}; w::NTuple{3,T}
    lens_radius::T
end
CCamera(c::Camera{T}) where T = CCamera{T}(Tuple(c.origin), Tuple(c.lower_left_corner), Tuple(c.horizontal),
                                           Tuple(c.vertical), Tuple(c.u), Tuple(c.v), Tuple(c.w), c.lens_radius)

# rtw_params (ABI version 3: same layout as version 2; new flag bits)
struct CParams
    width::Int32; height::Int32; spp::Int32; max_depth::Int32
    seed::UInt64
    n_chunks::Int32; shard_index::Int32; shard_count::Int32; device::Int32; gamma::Int32; flags::Int32
    n_devices::Int32; job_pixels::Int32
    device_ids::Ptr{Int32}
end

function __init__()
    v = ccall((:rtw_abi_version, LIB), Cint, ())
    v == 4 || error("librtw_hip.so has ABI version $v; this shim binds version 4 (include/rtw_hip.h)")
end

matkind(::Lambertian) = Int32(0)
matkind(::Metal) = Int32(1)
matkind(::Dielectric) = Int32(2)
matkind(m) = throw(ArgumentError("unsupported material $(typeof(m)) on the HIP path"))
albedo(m::Lambertian{T}) where T = m.albedo
albedo(m::Metal{T}) where T = m.albedo
albedo(::Dielectric{T}) where T = SVector{3,T}(1, 1, 1)
matparam(::Lambertian{T}) where T = zero(T)
matparam(m::Metal{T}) where T = m.fuzz
matparam(m::Dielectric{T}) where T = m.ir

last_error() = unsafe_string(ccall((:rtw_last_error, LIB), Cstring, ()))

"""
    render(scene, cam, image_width=400, n_samples=1; depth=16, seed=1, n_chunks=0, device=-1, devices=nothing, numerics=:reference, group_cull=false, scan_valu=false, ray_pool=false, rccl_reduce=false)

Drop-in for `RayTracingWeekend.render` (src/render.jl:8-44) on MI355X.  Keyword extras only.
`depth=16` is the reference's hard-wired `ray_color` default (src/ray_color.jl:14).
`devices=:all` uses every visible GPU, `devices=[0, 1, 2]` the listed ones (the 8x8 tiles are dealt
round-robin to the devices inside the library; the image is identical for any device list).
`numerics` selects the deciding arithmetic of `hit(::Sphere)` (src/hit.jl:16-18): `:reference` (default) = the reference's own order -- StaticArrays' un-fused
`dot`, one rounding per written operation --, `:reference_fma2` = the same with both squares contracted, `disc = fma(half_b, half_b, -c)` and `c = fma(-r, r, oc⋅oc)`, `:contract` = three FMA chains
(RTW_FLAG_NUMERICS_*; in Float32 the choice moves the image mean by 0.003 and the work by 4 %: `tools/julia_kat.jl` tells which one this Julia build emits).
`group_cull=true` selects the opt-in culling scan (RTW_FLAG_GROUP_CULL), `scan_valu=true` the all-VALU form of either
scan (RTW_FLAG_SCAN_VALU, for A/B measurements): same image bit for bit in every mode; `ray_pool=true` (RTW_FLAG_RAY_POOL) needs a `make POOL=1` build of the library.
`rccl_reduce=true` (with `devices`): the shards are put together by one ncclReduce inside the library (RTW_FLAG_RCCL_REDUCE) instead of peer copies.
"""
function render(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1;
                depth=16, seed=1, n_chunks=0, device=-1, devices=nothing, numerics=:reference, group_cull=false, scan_valu=false, ray_pool=false, rccl_reduce=false) where T <: Union{Float32,Float64}
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0         # RTW_FLAG_NUMERICS_CONTRACT / _REFERENCE_FMA2
    image_height = image_width ÷ (16//9)                       # src/render.jl:11-12
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    img = Matrix{RGB{T}}(undef, image_height, image_width)      # column-major H x W, 3 x T per pixel
    ccam = Ref(CCamera(cam))
    ids = devices isa AbstractVector ? Int32.(devices) : Int32[]
    n_devices = devices === :all ? -1 : (length(ids) > 1 ? length(ids) : 0)
    length(ids) == 1 && (device = ids[1])
    rc = GC.@preserve cx cy cz r kind ar ag ab param img ids begin
        params = Ref(CParams(image_width, image_height, n_samples, depth, seed, n_chunks, 0, 1, device, 1, (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | (ray_pool ? 8 : 0) | (rccl_reduce ? 16 : 0) | nflags,
                             n_devices, 0, length(ids) > 1 ? pointer(ids) : Ptr{Int32}(C_NULL)))
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        if T === Float32
            ccall((:rtw_render_f32, LIB), Cint, (Ref{CScene{Float32}}, Ref{CCamera{Float32}}, Ref{CParams}, Ptr{Float32}),
                  cscene, ccam, params, pointer(reinterpret(Float32, vec(img))))
        else
            ccall((:rtw_render_f64, LIB), Cint, (Ref{CScene{Float64}}, Ref{CCamera{Float64}}, Ref{CParams}, Ptr{Float64}),
                  cscene, ccam, params, pointer(reinterpret(Float64, vec(img))))
        end
    end
    rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    img
end

"""
    render(scene, cams::AbstractVector{Camera{T}}, image_width=400, n_samples=1; depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false)

Batched render (rtw_render_batch_f32/_f64): every camera of `cams` in ONE kernel launch on one device.  Returns an
`Array{RGB{T},3}` of size (image_height, image_width, length(cams)); `img[:, :, v]` is bit-identical to
`render(scene, cams[v], image_width, n_samples; seed=seeds[v])`.  `seed`: one integer for every view or a vector of `length(cams)`.
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_batch.py drives the same entry point.)
"""
function render(scene::HittableList, cams::AbstractVector{Camera{T}}, image_width=400, n_samples=1;
                depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false) where T <: Union{Float32,Float64}
    isempty(cams) && throw(ArgumentError("cams is empty"))
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    nv = length(cams)
    seeds = seed isa Integer ? fill(UInt64(seed), nv) : UInt64.(seed)
    length(seeds) == nv || throw(ArgumentError("$(length(seeds)) seeds for $nv views"))
    image_height = image_width ÷ (16//9)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    img = Array{RGB{T},3}(undef, image_height, image_width, nv)     # view v = the v-th consecutive Matrix{RGB{T}}
    ccams = [CCamera(c) for c in cams]
    rc = GC.@preserve cx cy cz r kind ar ag ab param img ccams seeds begin
        params = Ref(CParams(image_width, image_height, n_samples, depth, seeds[1], n_chunks, 0, 1, device, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        if T === Float32
            ccall((:rtw_render_batch_f32, LIB), Cint, (Ref{CScene{Float32}}, Ptr{CCamera{Float32}}, Int32, Ptr{UInt64}, Ref{CParams}, Ptr{Float32}),
                  cscene, pointer(ccams), nv, pointer(seeds), params, pointer(reinterpret(Float32, vec(img))))
        else
            ccall((:rtw_render_batch_f64, LIB), Cint, (Ref{CScene{Float64}}, Ptr{CCamera{Float64}}, Int32, Ptr{UInt64}, Ref{CParams}, Ptr{Float64}),
                  cscene, pointer(ccams), nv, pointer(seeds), params, pointer(reinterpret(Float64, vec(img))))
        end
    end
    rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    img
end

# rtw_temporal_t (48 bytes) and rtw_temporal_clamp_t (32 bytes), include/rtw_hip.h
struct CTemporal
    normal_power_log2::Int32; flags::Int32; gamma::Int32; device::Int32; reserved::NTuple{2,Int32}
    sigma_depth::Float64; min_weight::Float64; history_max::Float64
end
struct CTemporalClamp
    radius::Int32; flags::Int32; reserved::NTuple{2,Int32}
    sigma::Float64; len_scale::Float64
end

"""
    render_sequence_clamped(scene, cams, image_width=400, n_samples=1; radius=1, guides=false, sigma=1.0, len_scale=1.0, depth=16, seed=1, device=-1)

A camera path with clamped history reuse (rtw_render_path_clamped_f32/_f64 with `n` and `d` NULL: no noise maps, no filter): one batched
render, one batched feature pass and `length(cams)` temporal steps whose reprojected history is clamped to mean ± `sigma` standard deviations
of the current frame's (2·radius+1)² window.  Returns an `Array{RGB{T},3}` like the batched `render`; the temporal step runs at the header's
defaults, the clamp's defaults are untuned (DESIGN.md 7.21).
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_temporal_clamp.py drives the same entry point.)
"""
function render_sequence_clamped(scene::HittableList, cams::AbstractVector{Camera{T}}, image_width=400, n_samples=1;
                                 radius=1, guides=false, sigma=1.0, len_scale=1.0, depth=16, seed=1, device=-1) where T <: Union{Float32,Float64}
    isempty(cams) && throw(ArgumentError("cams is empty"))
    nv = length(cams)
    seeds = seed isa Integer ? fill(UInt64(seed), nv) : UInt64.(seed)
    length(seeds) == nv || throw(ArgumentError("$(length(seeds)) seeds for $nv views"))
    image_height = image_width ÷ (16//9)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    img = Array{RGB{T},3}(undef, image_height, image_width, nv)
    ccams = [CCamera(c) for c in cams]
    rc = GC.@preserve cx cy cz r kind ar ag ab param img ccams seeds begin
        params = Ref(CParams(image_width, image_height, n_samples, depth, seeds[1], 0, 0, 1, device, 1, 0, 0, 0, Ptr{Int32}(C_NULL)))
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        t = Ref(CTemporal(1, 1, 1, -1, (0, 0), 0.1, 0.25, 16.0))            # the header's defaults; RTW_TEMPORAL_DEMODULATE
        c = Ref(CTemporalClamp(radius, guides ? 1 : 0, (0, 0), sigma, len_scale))       # RTW_CLAMP_GUIDES
        if T === Float32
            ccall((:rtw_render_path_clamped_f32, LIB), Cint, (Ref{CScene{Float32}}, Ptr{CCamera{Float32}}, Int32, Ptr{UInt64}, Ref{CParams}, Ref{CTemporal}, Ref{CTemporalClamp}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}),
                  cscene, pointer(ccams), nv, pointer(seeds), params, t, c, C_NULL, C_NULL, pointer(reinterpret(Float32, vec(img))))
        else
            ccall((:rtw_render_path_clamped_f64, LIB), Cint, (Ref{CScene{Float64}}, Ptr{CCamera{Float64}}, Int32, Ptr{UInt64}, Ref{CParams}, Ref{CTemporal}, Ref{CTemporalClamp}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}),
                  cscene, pointer(ccams), nv, pointer(seeds), params, t, c, C_NULL, C_NULL, pointer(reinterpret(Float64, vec(img))))
        end
    end
    rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    img
end

"""
    render_progressive(scene, cam, image_width=400, n_samples=1; passes=4, callback=nothing, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false)

Progressive render (rtw_render_accum_f32/_f64 into an rtw_accum): the render's chunks in `passes` passes of (nearly) equal chunk counts
on one device.  The returned `Matrix{RGB{T}}` is bit-identical to `render(scene, cam, image_width, n_samples; ...)` with the same keywords.
`callback(img, samples_done)` runs after every pass with the image of the samples added so far (rtw_accum_resolve_host_*: it waits for
the pass); a `true` return value stops the render and that image is returned.  `n_chunks` keeps `render`'s default (min(n_samples, 256)
chunks); refinement in 1-sample steps beyond 256 samples: `n_chunks = n_samples`.
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_accum.py drives the same entry points.)
"""
function render_progressive(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1;
                            passes=4, callback=nothing, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false) where T <: Union{Float32,Float64}
    passes >= 1 || throw(ArgumentError("passes must be >= 1"))
    n_samples >= 1 || throw(ArgumentError("n_samples must be >= 1"))
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    image_height = image_width ÷ (16//9)
    # the effective chunks of the render (include/rtw_hip.h rtw_params.n_chunks): what chunk_begin / chunk_count count
    nch = min(n_chunks > 0 ? n_chunks : min(n_samples, 256), n_samples)
    cs = cld(n_samples, nch)
    nch = cld(n_samples, cs)
    passes = min(passes, nch)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    img = Matrix{RGB{T}}(undef, image_height, image_width)
    ccam = Ref(CCamera(cam))
    check(rc) = rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    hscene = Ref{Ptr{Cvoid}}(C_NULL)
    hacc = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve cx cy cz r kind ar ag ab param img begin
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        params = Ref(CParams(image_width, image_height, n_samples, depth, seed, n_chunks, 0, 1, -1, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        out = pointer(reinterpret(T, vec(img)))
        try
            if T === Float32
                check(ccall((:rtw_scene_upload_f32, LIB), Cint, (Ref{CScene{Float32}}, Cint, Ref{Ptr{Cvoid}}), cscene, device, hscene))
            else
                check(ccall((:rtw_scene_upload_f64, LIB), Cint, (Ref{CScene{Float64}}, Cint, Ref{Ptr{Cvoid}}), cscene, device, hscene))
            end
            check(ccall((:rtw_accum_create, LIB), Cint, (Cint, Int32, Int32, Ref{Ptr{Cvoid}}), device, image_width, image_height, hacc))
            done = 0
            for k in 0:passes-1
                b, e = k * nch ÷ passes, (k + 1) * nch ÷ passes
                if T === Float32
                    check(ccall((:rtw_render_accum_f32, LIB), Cint, (Ptr{Cvoid}, Ref{CCamera{Float32}}, Ref{CParams}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                hscene[], ccam, params, b, e - b, hacc[], C_NULL, C_NULL))
                else
                    check(ccall((:rtw_render_accum_f64, LIB), Cint, (Ptr{Cvoid}, Ref{CCamera{Float64}}, Ref{CParams}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                hscene[], ccam, params, b, e - b, hacc[], C_NULL, C_NULL))
                end
                done = min(n_samples, e * cs)                  # samples per pixel in the chunks [0, e)
                if callback !== nothing || k == passes - 1
                    if T === Float32
                        check(ccall((:rtw_accum_resolve_host_f32, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), hacc[], 1, out))
                    else
                        check(ccall((:rtw_accum_resolve_host_f64, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), hacc[], 1, out))
                    end
                    callback !== nothing && callback(img, done) === true && break
                end
            end
        finally
            ccall((:rtw_accum_free, LIB), Cint, (Ptr{Cvoid},), hacc[])        # (NULL handles are accepted)
            ccall((:rtw_scene_free, LIB), Cint, (Ptr{Cvoid},), hscene[])
        end
    end
    img
end

struct CAdaptive
    tolerance::Float64; dark_floor::Float64
    min_chunks::Int32; check_chunks::Int32
    reserved::NTuple{2,Int32}
end

"""
    render_adaptive(scene, cam, image_width=400, n_samples=1; tolerance, dark_floor=0.03, min_chunks=0, check_chunks=0, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false)

Adaptive sampling (rtw_render_adaptive_f32/_f64): at most `n_samples` samples per pixel; every 8x8 tile stops at the first checkpoint at
which it is converged under `tolerance` (roughly 0.8 x the tile's relative standard error; the exact rule is in include/rtw_hip.h).
Returns `(img, tile_chunks)`: the `Matrix{RGB{T}}`, each pixel divided by the samples its tile holds, and the `tiles_i x tiles_j` matrix
of the chunk counts C_t -- tile (ti, tj) of `img` is bit-identical to `render(...; n_chunks=C_t)` with `min(n_samples, C_t * chunk size)`
samples.  `dark_floor` (default 0.03 = 1 % of white: a choice, not a measurement) keeps near-black tiles from never stopping.
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_adaptive.py drives the same entry points.)
"""
function render_adaptive(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1;
                         tolerance, dark_floor=0.03, min_chunks=0, check_chunks=0, depth=16, seed=1, n_chunks=0, device=-1,
                         numerics=:reference, group_cull=false, scan_valu=false) where T <: Union{Float32,Float64}
    n_samples >= 1 || throw(ArgumentError("n_samples must be >= 1"))
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    image_height = image_width ÷ (16//9)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    img = Matrix{RGB{T}}(undef, image_height, image_width)
    tiles_i, tiles_j = cld(image_height, 8), cld(image_width, 8)
    chunks = Matrix{Int32}(undef, tiles_i, tiles_j)             # column-major like the tile numbering t = tj * tiles_i + ti
    ccam = Ref(CCamera(cam))
    check(rc) = rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    hscene = Ref{Ptr{Cvoid}}(C_NULL)
    hacc = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve cx cy cz r kind ar ag ab param img chunks begin
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        params = Ref(CParams(image_width, image_height, n_samples, depth, seed, n_chunks, 0, 1, -1, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        adaptive = Ref(CAdaptive(tolerance, dark_floor, min_chunks, check_chunks, (Int32(0), Int32(0))))
        out = pointer(reinterpret(T, vec(img)))
        try
            if T === Float32
                check(ccall((:rtw_scene_upload_f32, LIB), Cint, (Ref{CScene{Float32}}, Cint, Ref{Ptr{Cvoid}}), cscene, device, hscene))
            else
                check(ccall((:rtw_scene_upload_f64, LIB), Cint, (Ref{CScene{Float64}}, Cint, Ref{Ptr{Cvoid}}), cscene, device, hscene))
            end
            check(ccall((:rtw_accum_create, LIB), Cint, (Cint, Int32, Int32, Ref{Ptr{Cvoid}}), device, image_width, image_height, hacc))
            if T === Float32
                check(ccall((:rtw_render_adaptive_f32, LIB), Cint, (Ptr{Cvoid}, Ref{CCamera{Float32}}, Ref{CParams}, Ref{CAdaptive}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                            hscene[], ccam, params, adaptive, hacc[], C_NULL, C_NULL))
                check(ccall((:rtw_accum_resolve_host_f32, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), hacc[], 1, out))
            else
                check(ccall((:rtw_render_adaptive_f64, LIB), Cint, (Ptr{Cvoid}, Ref{CCamera{Float64}}, Ref{CParams}, Ref{CAdaptive}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                            hscene[], ccam, params, adaptive, hacc[], C_NULL, C_NULL))
                check(ccall((:rtw_accum_resolve_host_f64, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), hacc[], 1, out))
            end
            count = Ref{Int32}(0)
            check(ccall((:rtw_accum_tile_chunks, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Int32}), hacc[], length(chunks), count, pointer(chunks)))
        finally
            ccall((:rtw_accum_free, LIB), Cint, (Ptr{Cvoid},), hacc[])        # (NULL handles are accepted)
            ccall((:rtw_scene_free, LIB), Cint, (Ptr{Cvoid},), hscene[])
        end
    end
    img, chunks
end

# what the two batched methods below share: the scene uploaded once, one accumulator per camera, `body(hscene, haccs, params, ccams, seeds, check)`,
# and the handles freed whatever happens
function with_batch(body, scene::HittableList, cams::AbstractVector{Camera{T}}, image_width, n_samples, depth, seed, n_chunks, device,
                    numerics, group_cull, scan_valu) where T <: Union{Float32,Float64}
    isempty(cams) && throw(ArgumentError("cams is empty"))
    n_samples >= 1 || throw(ArgumentError("n_samples must be >= 1"))
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    nv = length(cams)
    seeds = seed isa Integer ? fill(UInt64(seed), nv) : UInt64.(seed)
    length(seeds) == nv || throw(ArgumentError("$(length(seeds)) seeds for $nv views"))
    image_height = image_width ÷ (16//9)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    ccams = [CCamera(c) for c in cams]
    check(rc) = rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    hscene = Ref{Ptr{Cvoid}}(C_NULL)
    haccs = fill(Ptr{Cvoid}(C_NULL), nv)
    GC.@preserve cx cy cz r kind ar ag ab param ccams seeds haccs begin
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        params = Ref(CParams(image_width, image_height, n_samples, depth, seeds[1], n_chunks, 0, 1, -1, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        try
            if T === Float32
                check(ccall((:rtw_scene_upload_f32, LIB), Cint, (Ref{CScene{Float32}}, Cint, Ref{Ptr{Cvoid}}), cscene, device, hscene))
            else
                check(ccall((:rtw_scene_upload_f64, LIB), Cint, (Ref{CScene{Float64}}, Cint, Ref{Ptr{Cvoid}}), cscene, device, hscene))
            end
            for v in 1:nv
                h = Ref{Ptr{Cvoid}}(C_NULL)
                check(ccall((:rtw_accum_create, LIB), Cint, (Cint, Int32, Int32, Ref{Ptr{Cvoid}}), device, image_width, image_height, h))
                haccs[v] = h[]
            end
            body(hscene[], haccs, params, ccams, seeds, check)
        finally
            for h in haccs
                ccall((:rtw_accum_free, LIB), Cint, (Ptr{Cvoid},), h)          # (NULL handles are accepted)
            end
            ccall((:rtw_scene_free, LIB), Cint, (Ptr{Cvoid},), hscene[])
        end
    end
end

"""
    render_progressive(scene, cams::AbstractVector{Camera{T}}, image_width=400, n_samples=1; passes=4, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false)

Batched progressive render (rtw_render_accum_batch_f32/_f64): every camera of `cams` with an accumulator of its own, each of the `passes`
passes ONE kernel launch for all of them.  Returns an `Array{RGB{T},3}` of size (image_height, image_width, length(cams)); `img[:, :, v]`
is bit-identical to `render(scene, cams[v], image_width, n_samples; seed=seeds[v])`.  `seed`: one integer for every view or a vector.
(tests/test_gpu_accum_batch.py drives the same entry points through ctypes.)
"""
function render_progressive(scene::HittableList, cams::AbstractVector{Camera{T}}, image_width=400, n_samples=1;
                            passes=4, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false) where T <: Union{Float32,Float64}
    passes >= 1 || throw(ArgumentError("passes must be >= 1"))
    nv = length(cams)
    image_height = image_width ÷ (16//9)
    nch = min(n_chunks > 0 ? n_chunks : min(n_samples, 256), n_samples)      # the effective chunks (include/rtw_hip.h rtw_params.n_chunks)
    nch = cld(n_samples, cld(n_samples, nch))
    passes = min(passes, nch)
    img = Array{RGB{T},3}(undef, image_height, image_width, nv)
    with_batch(scene, cams, image_width, n_samples, depth, seed, n_chunks, device, numerics, group_cull, scan_valu) do hscene, haccs, params, ccams, seeds, check
        GC.@preserve img begin
            for k in 0:passes-1
                b, e = k * nch ÷ passes, (k + 1) * nch ÷ passes
                if T === Float32
                    check(ccall((:rtw_render_accum_batch_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{CCamera{Float32}}, Int32, Ptr{UInt64}, Ref{CParams}, Int32, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}),
                                hscene, pointer(ccams), nv, pointer(seeds), params, b, e - b, pointer(haccs), C_NULL, C_NULL))
                else
                    check(ccall((:rtw_render_accum_batch_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{CCamera{Float64}}, Int32, Ptr{UInt64}, Ref{CParams}, Int32, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}),
                                hscene, pointer(ccams), nv, pointer(seeds), params, b, e - b, pointer(haccs), C_NULL, C_NULL))
                end
            end
            for v in 1:nv
                out = pointer(reinterpret(T, vec(img))) + (v - 1) * image_height * image_width * 3 * sizeof(T)
                if T === Float32
                    check(ccall((:rtw_accum_resolve_host_f32, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), haccs[v], 1, out))
                else
                    check(ccall((:rtw_accum_resolve_host_f64, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), haccs[v], 1, out))
                end
            end
        end
    end
    img
end

"""
    render_adaptive(scene, cams::AbstractVector{Camera{T}}, image_width=400, n_samples=1; tolerance, dark_floor=0.03, min_chunks=0, check_chunks=0, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false)

Batched adaptive sampling (rtw_render_adaptive_batch_f32/_f64): every camera of `cams` in ONE loop of passes -- per checkpoint one check,
one list of the active tiles of all views, one host wait, one launch.  Returns `(img, tile_chunks)`: an `Array{RGB{T},3}` of size
(image_height, image_width, length(cams)) and an `Array{Int32,3}` of size (tiles_i, tiles_j, length(cams)); view `v` of both is
bit-identical to `render_adaptive(scene, cams[v], ...; seed=seeds[v])`.  `seed`: one integer for every view or a vector.
(tests/test_gpu_accum_batch.py drives the same entry points through ctypes.)
"""
function render_adaptive(scene::HittableList, cams::AbstractVector{Camera{T}}, image_width=400, n_samples=1;
                         tolerance, dark_floor=0.03, min_chunks=0, check_chunks=0, depth=16, seed=1, n_chunks=0, device=-1,
                         numerics=:reference, group_cull=false, scan_valu=false) where T <: Union{Float32,Float64}
    nv = length(cams)
    image_height = image_width ÷ (16//9)
    tiles_i, tiles_j = cld(image_height, 8), cld(image_width, 8)
    img = Array{RGB{T},3}(undef, image_height, image_width, nv)
    chunks = Array{Int32,3}(undef, tiles_i, tiles_j, nv)          # view v: column-major like the tile numbering t = tj * tiles_i + ti
    with_batch(scene, cams, image_width, n_samples, depth, seed, n_chunks, device, numerics, group_cull, scan_valu) do hscene, haccs, params, ccams, seeds, check
        adaptive = Ref(CAdaptive(tolerance, dark_floor, min_chunks, check_chunks, (Int32(0), Int32(0))))
        GC.@preserve img chunks begin
            if T === Float32
                check(ccall((:rtw_render_adaptive_batch_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{CCamera{Float32}}, Int32, Ptr{UInt64}, Ref{CParams}, Ref{CAdaptive}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}),
                            hscene, pointer(ccams), nv, pointer(seeds), params, adaptive, pointer(haccs), C_NULL, C_NULL))
            else
                check(ccall((:rtw_render_adaptive_batch_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{CCamera{Float64}}, Int32, Ptr{UInt64}, Ref{CParams}, Ref{CAdaptive}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}),
                            hscene, pointer(ccams), nv, pointer(seeds), params, adaptive, pointer(haccs), C_NULL, C_NULL))
            end
            count = Ref{Int32}(0)
            for v in 1:nv
                out = pointer(reinterpret(T, vec(img))) + (v - 1) * image_height * image_width * 3 * sizeof(T)
                if T === Float32
                    check(ccall((:rtw_accum_resolve_host_f32, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), haccs[v], 1, out))
                else
                    check(ccall((:rtw_accum_resolve_host_f64, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), haccs[v], 1, out))
                end
                check(ccall((:rtw_accum_tile_chunks, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Int32}), haccs[v], tiles_i * tiles_j, count,
                            pointer(chunks) + (v - 1) * tiles_i * tiles_j * sizeof(Int32)))
            end
        end
    end
    img, chunks
end

"""
    render_features(scene, cam, image_width=400, n_samples=1; seed=1, n_chunks=0, chunks=nothing, device=-1, numerics=:reference, group_cull=false, scan_valu=false)

First-hit feature buffers (rtw_render_features_f32/_f64) of the render `render(scene, cam, image_width, n_samples; seed, n_chunks)`: an
`Array{T,3}` of size (8, image_height, image_width) -- per pixel `[1:3]` albedo (the sky colour where nothing is hit), `[4:6]` the
face-forwarded normal, `[7]` depth (t), `[8]` coverage, each the mean over the primary rays of the chunks' first samples (normals are not
renormalised, depth is averaged over hits and misses alike: divide both by the coverage).  `chunks=nothing`: the whole render;
`chunks=(begin, count)`: that range of its effective chunks (0-based, as in `render_progressive`).  A poisoned pixel is NaN in all 8 slots.
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_features.py drives the same entry point.)
"""
function render_features(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1;
                         seed=1, n_chunks=0, chunks=nothing, device=-1, numerics=:reference, group_cull=false, scan_valu=false) where T <: Union{Float32,Float64}
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    image_height = image_width ÷ (16//9)
    # the effective chunks of the render under the default rule of rtw_params.n_chunks
    nch = min(n_chunks > 0 ? n_chunks : min(n_samples, 256), n_samples)
    chunk_spp = cld(n_samples, nch)
    chunk_begin, chunk_count = chunks === nothing ? (0, cld(n_samples, chunk_spp)) : chunks
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    out = Array{T,3}(undef, 8, image_height, image_width)       # RTW_FEATURE_CHANNELS values per pixel, pixels column-major
    ccam = Ref(CCamera(cam))
    rc = GC.@preserve cx cy cz r kind ar ag ab param out begin
        params = Ref(CParams(image_width, image_height, n_samples, 16, seed, n_chunks, 0, 1, device, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        if T === Float32
            ccall((:rtw_render_features_f32, LIB), Cint, (Ref{CScene{Float32}}, Ref{CCamera{Float32}}, Ref{CParams}, Int32, Int32, Ptr{Float32}),
                  cscene, ccam, params, chunk_begin, chunk_count, pointer(out))
        else
            ccall((:rtw_render_features_f64, LIB), Cint, (Ref{CScene{Float64}}, Ref{CCamera{Float64}}, Ref{CParams}, Int32, Int32, Ptr{Float64}),
                  cscene, ccam, params, chunk_begin, chunk_count, pointer(out))
        end
    end
    rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    out
end

# rtw_denoise_t (include/rtw_hip.h): 40 bytes
struct CDenoise
    levels::Int32; normal_power_log2::Int32; flags::Int32; gamma::Int32; device::Int32; reserved::Int32
    sigma_color::Float64; sigma_depth::Float64
end

"""
    render_denoised(scene, cam, image_width=400, n_samples=1; depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false,
                    levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, demodulate=true)

`render` at a low sample count through the feature-guided denoiser (rtw_render_denoised_f32/_f64): the linear image, the first-hit feature
pass over all of its chunks and an edge-avoiding à-trous filter (`levels` passes with steps 1, 2, 4, ...; colour, normal, relative-depth
and coverage weights; the definition is in include/rtw_hip.h) run on the device, gamma is applied at the end and the `Matrix{RGB{T}}`
comes back once.  `demodulate=true` filters image / albedo and multiplies the albedo back (RTW_DENOISE_DEMODULATE).
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_denoise.py drives the same entry point.)
"""
function render_denoised(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1;
                         depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false,
                         levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, demodulate=true) where T <: Union{Float32,Float64}
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    image_height = image_width ÷ (16//9)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    img = Matrix{RGB{T}}(undef, image_height, image_width)
    ccam = Ref(CCamera(cam))
    den = Ref(CDenoise(levels, normal_power_log2, demodulate ? 1 : 0, 1, -1, 0, sigma_color, sigma_depth))
    rc = GC.@preserve cx cy cz r kind ar ag ab param img begin
        params = Ref(CParams(image_width, image_height, n_samples, depth, seed, n_chunks, 0, 1, device, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        if T === Float32
            ccall((:rtw_render_denoised_f32, LIB), Cint, (Ref{CScene{Float32}}, Ref{CCamera{Float32}}, Ref{CParams}, Ref{CDenoise}, Ptr{Float32}),
                  cscene, ccam, params, den, pointer(reinterpret(Float32, vec(img))))
        else
            ccall((:rtw_render_denoised_f64, LIB), Cint, (Ref{CScene{Float64}}, Ref{CCamera{Float64}}, Ref{CParams}, Ref{CDenoise}, Ptr{Float64}),
                  cscene, ccam, params, den, pointer(reinterpret(Float64, vec(img))))
        end
    end
    rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    img
end

# rtw_upsample_t (include/rtw_hip.h): 48 bytes
struct CUpsample
    levels::Int32; normal_power_log2::Int32; flags::Int32; gamma::Int32; device::Int32; hi_chunks::Int32
    sigma_color::Float64; sigma_depth::Float64; sigma_albedo::Float64
end

"""
    render_upsampled(scene, cam, image_width=400, n_samples=1; lo_width=cld(image_width, 2), hi_chunks=0, depth=16, seed=1, n_chunks=0, device=-1,
                     numerics=:reference, group_cull=false, scan_valu=false, levels=2, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1,
                     sigma_albedo=0.2, demodulate=true)

A full-size frame from a render at `lo_width` (rtw_render_upsampled_f32/_f64): the small linear image, its feature pass, the feature pass
of the full frame over its first `hi_chunks` chunks (0: all) and the feature-guided upsampler (the definition is in include/rtw_hip.h) run
on the device, gamma is applied at the end and the full-size `Matrix{RGB{T}}` comes back once.  The filter's defaults are untuned.
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_upsample.py drives the same entry point.)
"""
function render_upsampled(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1;
                          lo_width=cld(image_width, 2), hi_chunks=0, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference,
                          group_cull=false, scan_valu=false, levels=2, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1,
                          sigma_albedo=0.2, demodulate=true) where T <: Union{Float32,Float64}
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    image_height = image_width ÷ (16//9)
    lo_height = lo_width ÷ (16//9)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    img = Matrix{RGB{T}}(undef, image_height, image_width)
    ccam = Ref(CCamera(cam))
    up = Ref(CUpsample(levels, normal_power_log2, demodulate ? 1 : 0, 1, -1, hi_chunks, sigma_color, sigma_depth, sigma_albedo))
    rc = GC.@preserve cx cy cz r kind ar ag ab param img begin
        params = Ref(CParams(image_width, image_height, n_samples, depth, seed, n_chunks, 0, 1, device, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        if T === Float32
            ccall((:rtw_render_upsampled_f32, LIB), Cint, (Ref{CScene{Float32}}, Ref{CCamera{Float32}}, Ref{CParams}, Int32, Int32, Ref{CUpsample}, Ptr{Float32}),
                  cscene, ccam, params, lo_width, lo_height, up, pointer(reinterpret(Float32, vec(img))))
        else
            ccall((:rtw_render_upsampled_f64, LIB), Cint, (Ref{CScene{Float64}}, Ref{CCamera{Float64}}, Ref{CParams}, Int32, Int32, Ref{CUpsample}, Ptr{Float64}),
                  cscene, ccam, params, lo_width, lo_height, up, pointer(reinterpret(Float64, vec(img))))
        end
    end
    rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    img
end

# rtw_present_t (include/rtw_hip.h): 32 bytes
struct CPresent
    channels::Int32; flags::Int32; device::Int32
    nan_rgb::NTuple{3,UInt8}; reserved0::UInt8
    exposure::Float64
    reserved::NTuple{2,Int32}
end

"""
    render_u8(scene, cam, image_width=400, n_samples=1; channels=3, dither=false, bgr=false, sqrt=false, exposure=1.0, nan_rgb=(0, 0, 0),
              denoise=false, depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false,
              levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, demodulate=true)

`render` (with `denoise=true`: `render_denoised`) and the present stage in one call (rtw_render_presented_f32/_f64): the float frame stays
on the device, where it is clipped, rounded in binary64 (ties to even; `dither=true`: an 8 × 8 ordered dither), packed and transposed, and
only the bytes come back.  Returns an `Array{UInt8,3}` of size `(channels, image_width, image_height)`: its memory is the row-major frame
a PNG or video writer takes -- channel k of pixel (i, j), 0-based, at `(i*image_width + j)*channels + k`; with the defaults the bytes are
`round(clamp(x, 0, 1) * 255)` of `render`'s image (the definition is in include/rtw_hip.h).
(Not executed in this repository: there is no `julia` in its build image; tests/test_gpu_present.py drives the same entry point.)
"""
function render_u8(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1;
                   channels=3, dither=false, bgr=false, sqrt=false, exposure=1.0, nan_rgb=(0, 0, 0), denoise=false,
                   depth=16, seed=1, n_chunks=0, device=-1, numerics=:reference, group_cull=false, scan_valu=false,
                   levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, demodulate=true) where T <: Union{Float32,Float64}
    numerics in (:reference, :contract, :reference_fma2) || throw(ArgumentError("numerics must be :reference, :contract or :reference_fma2"))
    channels in (3, 4) || throw(ArgumentError("channels must be 3 or 4"))
    nflags = numerics === :contract ? 32 : numerics === :reference_fma2 ? 128 : 0
    image_height = image_width ÷ (16//9)
    n = length(scene)
    cx = Vector{T}(undef, n); cy = similar(cx); cz = similar(cx); r = similar(cx)
    ar = similar(cx); ag = similar(cx); ab = similar(cx); param = similar(cx)
    kind = Vector{Int32}(undef, n)
    for (i, h) in enumerate(scene)
        h isa Sphere{T} || throw(ArgumentError("scene[$i] is $(typeof(h)); the HIP path takes Sphere{$T} only"))
        cx[i], cy[i], cz[i] = h.center
        r[i] = h.radius
        kind[i] = matkind(h.mat)
        ar[i], ag[i], ab[i] = albedo(h.mat)
        param[i] = matparam(h.mat)
    end
    bytes = Array{UInt8,3}(undef, channels, image_width, image_height)
    ccam = Ref(CCamera(cam))
    den = Ref(CDenoise(levels, normal_power_log2, demodulate ? 1 : 0, 1, -1, 0, sigma_color, sigma_depth))
    pres = Ref(CPresent(channels, (dither ? 1 : 0) | (bgr ? 2 : 0) | (sqrt ? 4 : 0), -1, UInt8.(Tuple(nan_rgb)), 0x00, exposure, (Int32(0), Int32(0))))
    rc = GC.@preserve cx cy cz r kind ar ag ab param bytes den begin
        params = Ref(CParams(image_width, image_height, n_samples, depth, seed, n_chunks, 0, 1, device, 1,
                             (group_cull ? 1 : 0) | (scan_valu ? 4 : 0) | nflags, 0, 0, Ptr{Int32}(C_NULL)))
        cscene = Ref(CScene{T}(n, pointer(cx), pointer(cy), pointer(cz), pointer(r), pointer(kind),
                               pointer(ar), pointer(ag), pointer(ab), pointer(param)))
        pden = denoise ? Base.unsafe_convert(Ptr{CDenoise}, den) : Ptr{CDenoise}(C_NULL)     # NULL: no filter
        if T === Float32
            ccall((:rtw_render_presented_f32, LIB), Cint, (Ref{CScene{Float32}}, Ref{CCamera{Float32}}, Ref{CParams}, Ptr{CDenoise}, Ref{CPresent}, Ptr{UInt8}),
                  cscene, ccam, params, pden, pres, pointer(bytes))
        else
            ccall((:rtw_render_presented_f64, LIB), Cint, (Ref{CScene{Float64}}, Ref{CCamera{Float64}}, Ref{CParams}, Ptr{CDenoise}, Ref{CPresent}, Ptr{UInt8}),
                  cscene, ccam, params, pden, pres, pointer(bytes))
        end
    end
    rc == 0 || error("librtw_hip: error $rc: $(last_error())")
    bytes
end

end # module
