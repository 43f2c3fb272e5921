// rtw_temporal_project.inc -- the ONE copy of the projection of a temporal step, included as text where it runs: tp_step (rtw_temporal.hpp),
// tp_step_clamped (rtw_temporal_clamp.hpp) and the motion blur's velocity kernel (rtw_motion_blur.hpp: mb_previous).  As text and not as a
// function because the step kernels must keep their instructions: a function of the same arithmetic changed the order of independent
// instructions in 16 of the 48 step instances (tools/isa_compare.py; profiles/motion_blur_isa_compare.txt), this does not.
// Reads from the including scope: T, V, MOTION (constexpr bool), U (TpParams<T>), i, j, W, H, P (long long), has (bool), z (T) and, with MOTION,
// B.plane (const V *).  Defines there: su, tv, D0..D2, sl, n0..n2 (the pixel's own ray), d0..d2 (the point to reproject, relative to the
// previous origin), dw, front, lam, s, t, x, y (its position in the previous view).
        // ---- the pixel's own ray in the current camera (the centre of the trace kernel's samples; the lens is ignored)
        const T su = (T((int)j) + T(1.5)) / T((int)W);
        const T tv = (T((int)(H - i)) - T(0.5)) / T((int)H);
        const T D0 = ((U.llc[0] + su * U.hor[0]) + tv * U.ver[0]) - U.o[0];
        const T D1 = ((U.llc[1] + su * U.hor[1]) + tv * U.ver[1]) - U.o[1];
        const T D2 = ((U.llc[2] + su * U.hor[2]) + tv * U.ver[2]) - U.o[2];
        const T sl = dn_sqrt((D0 * D0 + D1 * D1) + D2 * D2);
        const T n0 = D0 / sl, n1 = D1 / sl, n2 = D2 / sl;
        // ---- the point to reproject (a sky pixel: the point at infinity), relative to the previous origin
        T d0, d1, d2;
        if constexpr (MOTION) {
            // where the surface was one frame ago: d = ((origin + z*nD) - m) - origin_prev (a non-finite m: d is NaN, inr fails, the pixel resets)
            const V mv = B.plane[P];
            d0 = has ? ((U.o[0] + z * n0) - mv.x) - U.po[0] : n0;
            d1 = has ? ((U.o[1] + z * n1) - mv.y) - U.po[1] : n1;
            d2 = has ? ((U.o[2] + z * n2) - mv.z) - U.po[2] : n2;
        } else {
            d0 = has ? (U.o[0] + z * n0) - U.po[0] : n0;
            d1 = has ? (U.o[1] + z * n1) - U.po[1] : n1;
            d2 = has ? (U.o[2] + z * n2) - U.po[2] : n2;
        }
        // ---- projection into the previous camera
        const T dw = tp_dot<T>(d0, d1, d2, U.pw);
        const bool front = dw < T(0);
        const T lam = U.Kw / dw;
        const T s = (lam * tp_dot<T>(d0, d1, d2, U.ph) - U.Qh) * U.ih;
        const T t = (lam * tp_dot<T>(d0, d1, d2, U.pv) - U.Qv) * U.iv;
        const T x = s * T((int)W) - T(1.5);
        const T y = (T((int)H) - T(0.5)) - t * T((int)H);
