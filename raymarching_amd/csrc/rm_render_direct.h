// rm_render_direct.h -- per-pixel render pipelines, one lane = one pixel.
//
// Straight control flow per lane (march, normal, probes, shadow march, ...).
// Lanes of a wave diverge only in loop trip counts; at 4096^2 the 8x8-pixel
// waves are coherent enough that 94 % of lane-steps are useful for scene T
// (tools/wave_sim.py on the oracle's per-pixel step traces), so a
// wave-compacted state machine would not pay for its phase switching.
#pragma once
#include "rm_device.h"
#include "rm_wire_tile.h"

namespace rm {

// Colour-only normalization (Phong's vectors, the indirect light's direction:
// v_rsq, every scene; ScenePolicy, rm_device.h)
__device__ __forceinline__ V3 cnormalize(V3 a) { return a * __builtin_amdgcn_rsqf(dot(a, a)); }
// the scene distance for marches and normals (exact for scene O), and for
// the AO / shadow / thickness probes, whose results are smooth in the distance
template <int SC, int NB = 3>
__device__ __forceinline__ float dist_march(const FrameConst& F, V3 p, Tally& cnt) {
    return scene_dist<SC, ScenePolicy<SC>::kExactMarch, NB>(F, p, cnt);
}
template <int SC, int NB = 3>
__device__ __forceinline__ float dist_probe(const FrameConst& F, V3 p, Tally& cnt) {
    return scene_dist<SC, kProbeForm, NB>(F, p, cnt);
}
// normals and light directions: v_rsq where the scene's marches use the hardware forms too
template <int SC>
__device__ __forceinline__ V3 mnormalize(V3 a) {
    if constexpr (ScenePolicy<SC>::kHwMath) return a * __builtin_amdgcn_rsqf(dot(a, a));
    else return normalize(a);
}

// Scene O's floor-plane spans (scene_dist_O's slack, rm_device.h).  Along a
// ray with a unit direction d the plane-only result holds for a parameter span
// slack / (1 + |d.y|) (1.01: directions up to 1 % off unit length); the probes
// of a shading point (normal 0.0018, AO <= 0.8, thickness < 1 away) are all
// plane-only when the slack there is >= 2.05.
__device__ __forceinline__ float plane_rate(V3 d) {  // (v_rcp: 1 ulp is far inside the margin)
    return __builtin_amdgcn_rcpf(1.01f + fabsf(d.y));
}
template <int SC>
__device__ __forceinline__ bool plane_probes(const FrameConst& F, V3 p) {
    if constexpr (ScenePolicy<SC>::kPlaneSpans) {
        Tally scratch;  // (not a ray-step of the reference)
        float slack;
        (void)scene_dist_O<kProbeForm>(p, sponge_space<kProbeForm>(F, p), scratch, slack);
        return slack >= 2.05f;
    } else {
        (void)F; (void)p;
        return false;
    }
}
// a probe's distance: EXACT = the march form (normals), else the probe form
template <int SC, bool EXACT, int NB = 3>
__device__ __forceinline__ float dist_at(const FrameConst& F, V3 p, Tally& cnt, bool plane) {
    if constexpr (ScenePolicy<SC>::kPlaneSpans) {
        if (plane) {
            cnt.evals++;
            return p.y;
        }
    }
    if constexpr (EXACT) return dist_march<SC, NB>(F, p, cnt);
    else return dist_probe<SC, NB>(F, p, cnt);
}

// Scene T's probes in a far-sky wave of the timed kernels (render_T_from, rm_far_sky.h): every
// lane's far point has max|q| >= kFarSkyFar = 4.1; the normal's probes lie 0.0018 from it and the AO probes at most
// 0.81 (4 * 0.2 |n|, |n| = 1 within 1e-6), and the rotation into sponge space does not lengthen a displacement, so
// every probe has box = max|q| - 1 >= 2.29 (roundings ~1e-5).  sponge_folds returns its d unchanged once d >= 1/3
// (its first exit test, on every lane of the wave): the probe's distance is its box term, and the exit compare,
// the ballot and the branch of each probe are not needed.  BOX = true states that (scene T only); the
// instrumented kernels keep the folds' path and its counts.
// common.frag:697-708 (tetrahedral gradient, h = 0.001)
template <int SC, int NB = 3, bool BOX = false>
__device__ __forceinline__ V3 normal_fast(const FrameConst& F, V3 p, Tally& cnt, bool plane = false) {
    static_assert(!BOX || SC == SCENE_T, "box-only probes: scene T's far-sky waves");
    const float h = 0.001f;
    auto dist = [&](V3 q) {
        if constexpr (BOX) return sponge_box(sponge_space<ScenePolicy<SC>::kExactMarch>(F, q));
        else return dist_at<SC, kExactForm, NB>(F, q, cnt, plane);
    };
    float d0 = dist(p + v3(h, -h, -h));
    float d1 = dist(p + v3(-h, -h, h));
    float d2 = dist(p + v3(-h, h, -h));
    float d3 = dist(p + v3(h, h, h));
    V3 g = v3(d0, -d0, -d0) + v3(-d1, -d1, d1);
    g = g + v3(-d2, d2, -d2);
    g = g + v3(d3, d3, d3);
    return mnormalize<SC>(g);
}

// common.frag:879-901. Returns dist (depth on hit, -1 on miss, last SDF value
// on step exhaustion) and the point whose SdResult is returned.  One exit
// test per step; at a hit depth is left as it was, so the hit flag and depth
// give the three outcomes after the loop.
template <int SC, bool INSIDE>
__device__ __forceinline__ float cast_ray_d(const FrameConst& F, V3 ro, V3 rd, V3& last_q, Tally& cnt) {
    float depth = ZNEAR;
    float res = 0.0f;
    bool hit = false;
    if constexpr (ScenePolicy<SC>::kPlaneSpans) {
        // depth < t_plane: sceneSDF is the floor plane, (ro + rd depth).y
        const float ia = plane_rate(rd);
        float t_plane = 0.0f, last = 0.0f;
        for (int i = 0; i < F.max_steps; i++) {
            if (depth < t_plane) {
                res = ro.y + rd.y * depth;
                cnt.evals++;
                cnt.flop += 2;
            } else {
                V3 q = ro + rd * depth;
                float slack;
                cnt.flop += FL_TRANSFORM;
                res = scene_dist_O<kExactForm>(q, sponge_space<kExactForm>(F, q), cnt, slack);
                t_plane = depth + slack * ia;
            }
            last = depth;
            if (INSIDE) {
                hit = -res < 0.001f * depth;
                depth = hit ? depth : depth - res;
            } else {
                hit = res < 0.001f * depth;
                depth = hit ? depth : depth + res;
            }
            if (hit | (depth >= ZFAR)) break;
        }
        last_q = ro + rd * last;  // the point of the last step (ro without steps)
        return hit ? depth : depth >= ZFAR ? -1.0f : res;
    }
    last_q = ro;
    for (int i = 0; i < F.max_steps; i++) {
        V3 q = ro + rd * depth;
        res = dist_march<SC>(F, q, cnt);
        last_q = q;
        if (INSIDE) {  // castRayDI, common.frag:903-925
            hit = -res < 0.001f * depth;
            depth = hit ? depth : depth - res;
        } else {
            hit = res < 0.001f * depth;
            depth = hit ? depth : depth + res;
        }
        if (hit | (depth >= ZFAR)) break;
    }
    return hit ? depth : depth >= ZFAR ? -1.0f : res;
}

// The soft-shadow loops compute P = 2h for the next step before the exit
// test and pin it there (an empty asm): left free, the compiler sinks the add
// into a "continue" block of its own, which costs 4 SALU and 2 branches per
// step (C4 share 0.131 -> 0.119 ms, C2 P1 0.204 -> 0.188, scene O 4096^2
// 2.97 -> 2.92; profiles/r02/shadow_p_pin_ab.jsonl).
// Scene O's settle rule (soft_shadow2_T_loop states it for
// the sponge alone).  sceneSDF >= min(d0 - 0.33/6, d3 - 0.83/6, d1 - 1.33/6,
// d2 - 1.33/6) (each sminCubic lowers a min by at most k/6; output_shader.frag:
// 38-48 nests sphere d1 and cube d2, then the plane d3, then the sponge d0),
// with d0 >= the sponge's box term and d2 >= the cube's Chebyshev term.  Each
// of the four terms is convex along the ray (the plane linear), so it has an
// affine minorant through its value and a subgradient at t; their minimum
// minus the offsets, g, bounds every later h'.  If g >= 0.1 on [t, maxt]
// (checked at both ends: affine) every later step is unoccluded and, sceneSDF
// being 3-Lipschitz, h' / (2 ph) <= 0.665, so every later candidate is
// >= 4 * 0.7469 g(t') / t'; each g_i / t' is monotonic, so the minimum is at t
// or maxt: when 2.9 min(g(t) / t, g(maxt) / maxt) >= 1.01 res no later step
// changes res.  res^2 = 16 num / den (squared, as the loop keeps it).
// oracle settle_test_O restates the rule and checks it on every step of the
// reference's marches.
constexpr float kSettleK = (2.9f / 1.01f) * (2.9f / 1.01f) / 16.0f;  // both settle rules, squared: res^2 = 16 num / den
// (The slope of a Chebyshev term along the ray, d_i sign(q_i) on an axis
// attaining max_i |q_i|, is spelled out twice here and once in
// soft_shadow2_T_loop: as a shared function it compiled to other code.)
__device__ __forceinline__ bool shadow_settled_O(const LinRay& w, const LinRay& s, float t, float maxt, float num,
                                                 float den) {
    const float L = maxt - t;
    const V3 p = at(w, t), q = at(s, t);
    // sponge: box term in sponge space, slope along the sponge-space ray
    const float qx = fabsf(q.x), qy = fabsf(q.y), qm = fmaxf(qx, fmaxf(qy, fabsf(q.z)));
    const float sx = q.x < 0.0f ? -s.d.x : s.d.x, sy = q.y < 0.0f ? -s.d.y : s.d.y, sz = q.z < 0.0f ? -s.d.z : s.d.z;
    const float s0 = qx == qm ? sx : qy == qm ? sy : sz;
    const float a0 = qm - (1.0f + 0.33f / 6.0f);
    // sphere (3,2,3) r 1: |e| - 1, slope e.d / |e|
    const V3 e1 = p - v3(3.0f, 2.0f, 3.0f);
    const float l1 = __builtin_amdgcn_sqrtf(dot(e1, e1));
    const float a1 = l1 - (1.0f + 1.33f / 6.0f), s1 = dot(e1, w.d) * __builtin_amdgcn_rcpf(l1);
    // cube (-5,4,5) r 1: Chebyshev term
    const V3 e2 = p - v3(-5.0f, 4.0f, 5.0f);
    const float bx = fabsf(e2.x), by = fabsf(e2.y), bm = fmaxf(bx, fmaxf(by, fabsf(e2.z)));
    const float cx = e2.x < 0.0f ? -w.d.x : w.d.x, cy = e2.y < 0.0f ? -w.d.y : w.d.y, cz = e2.z < 0.0f ? -w.d.z : w.d.z;
    const float s2 = bx == bm ? cx : by == bm ? cy : cz;
    const float a2 = bm - (1.0f + 1.33f / 6.0f);
    const float a3 = p.y - 0.83f / 6.0f;  // plane
    const float g0 = fminf(fminf(a0, a1), fminf(a2, a3));
    const float g1 = fminf(fminf(fmaf(s0, L, a0), fmaf(s1, L, a1)), fminf(fmaf(s2, L, a2), fmaf(w.d.y, L, a3)));
    const float m = __builtin_elementwise_minimum(
        __builtin_elementwise_minimum(__builtin_elementwise_minimum(g0, g1) - 0.1f, kSettleK * g0 * g0 * den - num * t * t),
        kSettleK * g1 * g1 * den - num * maxt * maxt);
    return m >= 0.0f;
}

// A settled lane leaves at the test, and the uniform step cap is a branch of
// its own: the exit test does not materialize four booleans per step (C5
// frame 10.22 -> 10.03 ms; profiles/r03/scene_O_micro_ab.jsonl)
constexpr int kSettleOEvery = 8;  // steps between settle tests (a power of 2)

// common.frag:810-831, k = 4, for scenes O/OG: the probes step along the
// world ray and its sponge-space image, and the candidate is kept squared as
// in soft_shadow2_T below (the shadow factor is smooth in its roundings).
// SM as soft_shadow2_T_loop (0 none, 1 timed kernels: settle exit, 2
// instrumented kernels: every step taken, those after the settle point counted
// in cnt.skipped); O/OG only.  The settle test (~45 VALU) runs on every
// kSettleOEvery-th step: C5 frame 11.25 -> 10.51 ms with 8, 10.79 with 4
// (profiles/r03/scene_O_settle_ab.jsonl).
template <int SC, int SM = 0, bool CAP = true>
__device__ __forceinline__ float soft_shadow2_loop(const FrameConst& F, V3 ro, V3 rd, float mint, float maxt,
                                                   Tally& cnt) {
    constexpr bool kSettle = ScenePolicy<SC>::kSettleO && SM != 0;
    const LinRay w{ro, rd}, s = sponge_ray(F, ro, rd);
    float num = 1.0f / 16.0f, den = 1.0f, P = 0.0f, h = 1.0f;  // res = 1, k = 4
    float t = mint;
    const float ia = plane_rate(rd);
    float t_plane = 0.0f;  // t < t_plane: sceneSDF is the floor plane (O/OG)
    bool was_settled = false;  // SM == 2
    for (int it = 1; it == 1 ? t < maxt : true; it++) {
        if constexpr (SM == 2) cnt.skipped += was_settled ? 1u : 0u;
        if constexpr (SC == SCENE_PLUGIN) {
            h = dist_probe<SC>(F, at(w, t), cnt);
        } else if (t < t_plane) {
            h = fmaf(w.d.y, t, w.o.y);  // at(w, t).y
            cnt.evals++;
            cnt.flop += 2;
        } else {
            float slack;
            cnt.flop += FL_LINRAY;
            h = scene_dist_O<kProbeForm>(at(w, t), at(s, t), cnt, slack);
            t_plane = t + slack * ia;
        }
        float h2 = h * h;
        float Q = it == 1 ? 1.0f : fmaf(P, P, -h2);
        float D = it == 1 ? t : fmaf(t, P, -h2);
        float cn = h2 * Q, cd = D * fabsf(D);  // D <= 0: cd <= 0 fails the test (cn, den >= 0)
        bool upd = (Q >= 0.0f) & (cn * den < num * cd);
        num = upd ? cn : num;
        den = upd ? cd : den;
        bool settled = false;
        if constexpr (kSettle) {  // every kSettleOEvery-th step (h >= 0.1 is implied by the rule; h >= ph: moving away)
            if ((it & (kSettleOEvery - 1)) == 0 && __builtin_amdgcn_ballot_w64((h >= 0.1f) & (h + h >= P)) != 0)
                settled = (h >= 0.1f) & shadow_settled_O(w, s, t, maxt, num, den);
            // (a settled lane leaves here: its result needs neither P nor t)
            if constexpr (SM == 1) {
                if (settled) break;
            }
        }
        P = h + h;
        asm volatile("" : "+v"(P));  // keep P's add in the step (not in a continue block of its own)
        t += h * 0.1f + 0.001f;  // the reference's roundings: the step count is part of parity
        if constexpr (SM == 2) {
            was_settled |= settled;
            settled = false;
        }
        if ((h < 0.001f) | !(t < maxt)) break;
        if (CAP && it >= F.shadow_max_steps) break;  // (wave-uniform)
    }
    return h < 0.001f ? 0.0f : sqrtf(16.0f * num / den);
}
// The reference's uncapped march (the default) runs as a loop copy without
// the step-cap test, as scene T's (soft_shadow2_T).  Round 3
// measured no gain while the kernel spilled; without spills: C5 frame
// 8.524 -> 8.510 ms, C5 share 1.082 -> 1.077, O 4096^2 2.219 -> 2.212, frames
// identical (profiles/r05/ab_O_uncapped.jsonl)
template <int SC, int SM = 0>
__device__ __forceinline__ float soft_shadow2(const FrameConst& F, V3 ro, V3 rd, float mint, float maxt,
                                              Tally& cnt) {
    if (F.shadow_max_steps == __INT_MAX__) return soft_shadow2_loop<SC, SM, false>(F, ro, rd, mint, maxt, cnt);
    return soft_shadow2_loop<SC, SM, true>(F, ro, rd, mint, maxt, cnt);
}

// softShadow2 for scene T (fast math), stepping in sponge space and free of
// divisions and square roots.  With P = 2 ph the reference's y = h^2/P gives
//   k sqrt(h^2 - y^2) / (t - y) = k h sqrt(P^2 - h^2) / (t P - h^2),
// and res^2 / k^2 is kept as num/den, candidates h^2 Q / D^2 compared by
// cross-products (branch-free selects; D |D| for D^2 makes t - y <= 0 fail the
// comparison without a test of its own).  Candidates with t - y <= 0 (k d / 0:
// inf or NaN) or h^2 < y^2 (sqrt NaN) never lower res, as GLSL
// min(res, x) = x < res ? x : res.  On the first step ph = 1e20 makes y
// vanish: the candidate is k h / t (Q = 1, D = t below).  The occlusion result
// is recovered after the loop from the last h (a lane leaves through
// t >= maxt only with h >= 0.001).
//
// SETTLE (the timed kernels): a lane leaves the march as soon
// as no later step can change its result.  Every later step t' has h' >= B(t')
// (the sponge's box term, a lower bound of mengersponge), and B along the
// sponge-space ray, max_i |o_i + d_i t'| - 1, is convex: B(t') >= g(t') =
// B(t) + s (t' - t) with s = d_i sign(q_i) on an axis attaining the max.  If
// B(t) >= 0.1 and s >= 0, every later h' >= 0.1 (no occlusion) and the
// previous h >= 0.1, so with mengersponge 3-Lipschitz and the step 0.1 ph +
// 0.001, h' / (2 ph) <= 0.665 and every later candidate
// k h' sqrt(1 - (h'/2ph)^2) / (t' - y) is >= 4 * 0.7469 g(t') / t'.  g / t'
// is monotonic, so its minimum over [t, maxt] is at an endpoint: when
// 2.9 min(B / t, g(maxt) / maxt) >= 1.01 res no later candidate lowers res
// (margins far above the roundings), and the result is res now.  The test
// runs when some lane of the wave has B >= 0.1 and h >= ph (a march moving
// away from the sponge).  tools: oracle_shadow_settle checks the rule on every
// step of the reference's marches (no change of res after it, ever) and
// measures 43-55 % of scene T's shadow steps after it.  The instrumented
// kernels (COUNT) keep every step: their ray-step counts and maps are the
// reference's.
// (The candidate update is soft_shadow2_loop's and the slope on the axis
// attaining the Chebyshev max is shadow_settled_O's, restated: as shared
// functions they compiled to other code, here or in a scene plugin.  Change
// them together.)
// SM: 0 no settle test, 1 leave the march when settled (timed kernels), 2 run
// the test and count the steps after it in cnt.skipped (instrumented kernels:
// every reference step is still taken and counted)
// A settled lane leaves at the test, as in scene O's loop (C3 0.575 -> 0.568
// ms, C2 P1 0.192 -> 0.181); the test runs on every step.
// The settle gate is the AND of the two compares' own masks (s_and_b64) instead of a ballot of their combined i1, which the
// backend materialized as a 0/1 VGPR and a v_cmp_ne per step: 2 VALU fewer per
// shadow step, C3 0.4603-0.4626 -> 0.4527-0.4549 ms (profiles/r05/ab_settle_T.log)
template <bool CAP, int NB, int SM = 0>
__device__ __forceinline__ float soft_shadow2_T_loop(const FrameConst& F, const LinRay& s, float mint, float maxt,
                                                     Tally& cnt) {
    float num = 1.0f / 16.0f, den = 1.0f, P = 0.0f, h = 1.0f;  // res = 1, k = 4
    float t = mint;
    bool was_settled = false;  // SM == 2
    // one exit test per step (occluded, t >= maxt, settled, or the optional
    // step cap); t grows by >= 0.001 per continuing step, NaN leaves
    for (int it = 1; it == 1 ? t < maxt : true; it++) {
        const V3 q = at(s, t);
        const float box = sponge_box(q);
        cnt.evals++;
        cnt.flop += FL_LINRAY + FL_BOX;
        if constexpr (SM == 2) cnt.skipped += was_settled ? 1u : 0u;
        // The settle gate's two lane masks are taken where their operands are at hand: box >= 0.1 before the folds
        // raise the box term to h in place (box is not live across them; the settle block, which rarely runs, forms
        // it again from q), h + h >= P where P is last read (the new P is the old one's only successor).  Each
        // had cost a v_mov_b32 per step.
        const bool bfar = box >= 0.1f;
        const uint64_t m_far = SM != 0 ? __builtin_amdgcn_ballot_w64(bfar) : 0;
        h = sponge_folds<ScenePolicy<SCENE_T>::kExactMarch, NB>(q, box, cnt.flop);
        float h2 = h * h;
        float Q = it == 1 ? 1.0f : fmaf(P, P, -h2);
        float D = it == 1 ? t : fmaf(t, P, -h2);
        const bool away = h + h >= P;
        float cn = h2 * Q, cd = D * fabsf(D);  // D <= 0: cd <= 0 fails the test (cn, den >= 0)
        bool upd = (Q >= 0.0f) & (cn * den < num * cd);
        num = upd ? cn : num;
        den = upd ? cd : den;
        bool settled = false;
        if constexpr (SM != 0) {
            const bool any = (m_far & __builtin_amdgcn_ballot_w64(away)) != 0;
            if (any) {
                // sponge_box(q) again: the same operations, the same float (through an empty asm: left visible, the
                // compiler reuses the step's own max and box and keeps both live across the folds)
                float qx = q.x, qy = q.y, qz = q.z;
                asm volatile("" : "+v"(qx), "+v"(qy), "+v"(qz));
                const float ax = fabsf(qx), ay = fabsf(qy), m = fmaxf(ax, fmaxf(ay, fabsf(qz)));
                const float box = m - 1.0f;
                const float sx = qx < 0.0f ? -s.d.x : s.d.x, sy = qy < 0.0f ? -s.d.y : s.d.y;
                const float sz = qz < 0.0f ? -s.d.z : s.d.z;
                const float sl = ax == m ? sx : ay == m ? sy : sz;
                const float be = fmaf(sl, maxt - t, box);
                settled = bfar & away & (sl >= 0.0f) & (kSettleK * box * box * den >= num * t * t) &
                          (kSettleK * be * be * den >= num * maxt * maxt);
            }
        }
        if constexpr (SM == 1) {
            if (settled) break;  // (the result needs neither P nor t)
        }
        P = h + h;
        asm volatile("" : "+v"(P));  // keep P's add in the step (not in a continue block of its own)
        t = fmaf(h, 0.1f, t + 0.001f);
        if constexpr (SM == 2) {
            was_settled |= settled;
            settled = false;
        }
        if ((h < 0.001f) | !(t < maxt)) break;
        if (CAP && it >= F.shadow_max_steps) break;
    }
    return h < 0.001f ? 0.0f : __builtin_amdgcn_sqrtf(16.0f * num * __builtin_amdgcn_rcpf(den));
}
// The uncapped loop (the reference's, and the default) carries no step
// counter: a uniform counter test merged into the lanes' exit mask costs 5
// SALU per step, and SALU issue is a co-bottleneck of the kernel.
// (Scene O's soft_shadow2 has the same split since round 5.)
template <int NB = 3, int SETTLE = 0>
__device__ __forceinline__ float soft_shadow2_T(const FrameConst& F, const LinRay& s, float mint, float maxt,
                                                Tally& cnt) {
    if (F.shadow_max_steps == __INT_MAX__) return soft_shadow2_T_loop<false, NB, SETTLE>(F, s, mint, maxt, cnt);
    return soft_shadow2_T_loop<true, NB, SETTLE>(F, s, mint, maxt, cnt);
}

// castRay (common.frag:931-954) for scene T in sponge space; returns the
// depth of the point the reference returns (ZFAR on escape).  depth < ZFAR
// holds at a hit and after step exhaustion, so the escape value is set once,
// after the loop.
// RS, the reflection march of getColorReflect (common.frag:991-1002): its
// point only enters the colour as clamp(length(pr - p) / 3, 0, 1), and depth
// never decreases along the march, so once depth >= 3 (|pr - p| = 0.01 + depth
// within 1e-5) that factor is 1 whatever the march does next.  RS = 1 (timed
// kernels) leaves the march there; RS = 2 (instrumented) takes every step and
// counts those after it in cnt.skipped.
template <int NB = 3, int RS = 0>
__device__ __forceinline__ float cast_ray_T(const FrameConst& F, const LinRay& s, Tally& cnt) {
    constexpr float kStop = RS == 1 ? 3.0f : ZFAR;
    float depth = ZNEAR;
    for (int i = 0; i < F.max_steps; i++) {
        if constexpr (RS == 2) cnt.skipped += depth >= 3.0f ? 1u : 0u;
        float dist = menger_at<NB>(s, depth, cnt);
        bool hit = dist < 0.001f;
        depth = hit ? depth : depth + dist;
        if (hit | (depth >= kStop)) break;  // one exit test per step
    }
    return depth >= ZFAR ? ZFAR : depth;
}

// common.frag:850-866.  Scene O rolls the probe loop: the unrolled loop's
// interleaved probes spilled 18 VGPRs of the 8-wave kernel to scratch, rolled
// 4 (same frames, C5 frame 9.46 -> 9.43 ms; scene T's rolled loop measured
// 3 % slower, profiles/r03/rolled_probes_ab.jsonl)
// Scenes O/OG form the probe points of AO and thickness, and
// the sphere / cube lengths of the probe-form distance, with fused
// multiply-adds (these results are smooth in their roundings; the exact march
// and normal paths, and the thickness hash of the normal, keep the GLSL's):
// ScenePolicy<SC>::kProbeFma
__device__ __forceinline__ V3 fma3(V3 a, float s, V3 b) {  // a s + b, one rounding per component
    return v3(fmaf(a.x, s, b.x), fmaf(a.y, s, b.y), fmaf(a.z, s, b.z));
}
__device__ __forceinline__ float dot_fma(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }

// Scene T's four AO probes step along the normal's
// sponge-space image (q0 + (R n) 0.2 (i + 1), one FMA per axis) instead of
// transforming each probe point (the AO factor is smooth in the roundings;
// step counts do not depend on it)
// BOX (scene T's far-sky waves, normal_fast above): the probes' distances are their box terms
template <int SC, int NB = 3, bool BOX = false>
__device__ __forceinline__ float ao_real(const FrameConst& F, V3 pos, V3 n, Tally& cnt, bool plane = false) {
    static_assert(!BOX || SC == SCENE_T, "box-only probes: scene T's far-sky waves");
    float sum = 0.0f;
    if constexpr (SC == SCENE_T) {
        const LinRay r = sponge_ray(F, pos, n);
        auto dist = [&](float t) {
            if constexpr (BOX) return sponge_box(at(r, t));
            else return menger_at<NB>(r, t, cnt);
        };
#pragma unroll
        for (int i = 0; i < 4; i++) sum += (1.0f / (float)(1 << i)) * dist((float)(i + 1) * 0.2f);
        float maxSum = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++) maxSum += (1.0f / (float)(1 << i)) * (float)(i + 1) * 0.2f;
        return sum / maxSum;
    }
    auto probe = [&](int i) {
        V3 p = ScenePolicy<SC>::kProbeFma ? fma3(n, (float)(i + 1) * 0.2f, pos) : pos + (n * (float)(i + 1)) * 0.2f;
        sum += (1.0f / (float)(1 << i)) * dist_at<SC, kProbeForm, NB>(F, p, cnt, plane);
    };
    if constexpr (ScenePolicy<SC>::kPlaneSpans) {
#pragma unroll 1
        for (int i = 0; i < 4; i++) probe(i);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) probe(i);
    }
    // maxSum = sum_i 2^-i (i+1) 0.2, accumulated in f32 as the reference does
    float maxSum = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) maxSum += (1.0f / (float)(1 << i)) * (float)(i + 1) * 0.2f;
    return sum / maxSum;
}

// common.frag:730-754 (N = the caller's normal; L = normalize(lightPos - p),
// the caller's light direction, the same value)
__device__ __forceinline__ V3 phong(V3 k_d, V3 k_s, float alpha, V3 L, V3 p, V3 eye, V3 N) {
    V3 V = cnormalize(eye - p);
    V3 R = cnormalize(reflect(-L, N));
    float dotLN = dot(L, N);
    float dotRV = dot(R, V);
    if (dotLN < 0.0f) return v3s(0.0f);
    if (dotRV < 0.0f) return k_d * dotLN;
    return k_d * dotLN + k_s * gpow(dotRV, alpha);
}

// Soft shadows of points facing away from the light: phong returns 0 when
// dot(L, N) < 0 (common.frag:738-745), and the shadow factor only multiplies
// phong's term (template.frag:58,66; output_shader.frag:133,148),
// by shadow_pow(sha), finite for any sha in [0, 1]: the product
// is 0 whatever the march returns.  SM 1 (timed kernels) skips the march
// (sha = 1), SM 2 (instrumented) takes it and counts its steps in
// cnt.skipped, SM 0 takes it.  dotLN is phong's own dot(L, N): the same
// value, so the same decision.  Scene T at P0: 54 % of the shadow-march steps
// (oracle shadow_settle back_steps), scene O 0-6 % (its floor faces the light).
template <int SM, typename March>
__device__ __forceinline__ float shadow_if_lit(float dotLN, Tally& cnt, March march) {
    const bool lit = !(dotLN < 0.0f);
    if constexpr (SM == 1) {
        return lit ? march() : 1.0f;
    } else {
        const uint32_t e0 = cnt.evals, s0 = cnt.skipped;
        const float sha = march();
        if constexpr (SM == 2) {
            if (!lit) cnt.skipped = s0 + (cnt.evals - e0);
        }
        (void)e0; (void)s0; (void)lit;
        return sha;
    }
}

// pow(vec3(sha), vec3(1.0, 1.2, 1.5)): pow(x, 1) = x; one log2 shared by the other two
__device__ __forceinline__ V3 shadow_pow(float sha) {
    const float l = __builtin_amdgcn_logf(sha);
    return v3(sha, __builtin_amdgcn_exp2f(1.2f * l), __builtin_amdgcn_exp2f(1.5f * l));
}

// output_shader.frag:85-116
template <int SC>
__device__ __forceinline__ float thickness(const FrameConst& F, V3 pos, V3 norm, Tally& cnt, bool plane) {
    if constexpr (ScenePolicy<SC>::kPlaneSpans) {
        // A floor point whose probes are all plane-only: every sample is
        // pos.y + (sampleDir * sampleLength).y, and the sample directions depend
        // on the normal alone, which the floor's tetrahedral gradient makes
        // exactly (0, 1, 0) or (0, 1 - 2^-24, 0): per-frame tables (the host
        // evaluates GenerateSampleVector in GLSL float semantics).
        const bool n1 = norm.y == 1.0f;
        if (plane && norm.x == 0.0f && norm.z == 0.0f && (n1 || norm.y == 0x1.fffffep-1f)) {
            float th = 0.0f;
            for (int i = 0; i < 32; i++) th += F.hash11[i] + (pos.y + (n1 ? F.sss_floor[0][i] : F.sss_floor[1][i]));
            cnt.evals += 32;
            return clamp01(th * 0.03125f);
        }
    }
    float th = 0.0f;
    V3 nn = -norm;
    for (int i = 0; i < 32; i++) {
        float fi = (float)i;
        float sl = F.hash11[i];
        // the sample direction is not amplified (unlike the hash of the normal),
        // so it is normalized with v_rsq (~1 ulp) instead of a correctly
        // rounded sqrt and division: -22 VALU per sample, 32 samples
        const V3 hd = hash33(nn + v3s(fi)) - v3s(0.5f);
        if constexpr (ScenePolicy<SC>::kProbeFma) {
            const V3 rnd = hd * __builtin_amdgcn_rsqf(dot_fma(hd, hd));
            const V3 dir = fma3(nn * -2.0f, fminf(0.0f, dot_fma(rnd, nn)), rnd);  // reflectVector (:70-73)
            th += sl + dist_at<SC, kProbeForm>(F, fma3(dir, sl, pos), cnt, plane);
            continue;
        }
        V3 rnd = hd * __builtin_amdgcn_rsqf(dot(hd, hd));
        V3 dir = rnd - (nn * 2.0f) * fminf(0.0f, dot(rnd, nn));  // reflectVector (:70-73)
        th += sl + dist_at<SC, kProbeForm>(F, pos + dir * sl, cnt, plane);
    }
    return clamp01(th * 0.03125f);
}

// output_shader.frag:127-176.  The material of the hit (the SdResult at mq)
// is evaluated after the AO / shadow / thickness loops and returned in mat: it
// is not live across them (16 floats fewer in registers during the loops).
template <int SC, int SETTLE = 0>
__device__ __forceinline__ V3 light_O(const FrameConst& F, V3 mq, V3 ro, V3 rd, V3 p, V3 n, V3 phongN, bool plane,
                                     Mat& mat, Tally& cnt) {
    const V3 lightPos = v3(20.0f, 50.0f, 0.0f);
    V3 Ld = lightPos - p;
    V3 lightDir = normalize(Ld);
    float occ = ao_real<SC>(F, p, n, cnt, plane);
    float sha = shadow_if_lit<SETTLE>(dot(lightDir, phongN), cnt, [&] {
        return soft_shadow2<SC, SETTLE>(F, p, lightDir, 0.01f, length(Ld), cnt);
    });
    float th = thickness<SC>(F, p, n, cnt, plane);
    mat = scene_mat<SC>(F, mq);
    float sky = clamp01(0.5f + 0.5f * n.y);
    float ind = clamp01(dot(n, cnormalize(lightDir * v3(-1.0f, 0.0f, -1.0f))));
    V3 shading = phong(v3(1.64f, 1.27f, 0.99f), mat.specular, mat.shininess, lightDir, p, ro, phongN) * shadow_pow(sha);
    shading = shading + v3(0.16f, 0.20f, 0.28f) * sky * occ;
    shading = shading + v3(0.40f, 0.28f, 0.20f) * ind * occ;
    V3 sssl = lightDir + n * 0.6f;
    float sssdot = gpow(clamp01(dot(-rd, -sssl)), 1.1f) * 0.3f;
    shading = shading + v3s((sssdot + 0.3f) * th);
    V3 color = mat.diffuse * shading + mat.emission;
    return apply_scattering<ScenePolicy<SC>::kTrim>(color, ro, p);
}

// output_shader.frag:218-230
__device__ __forceinline__ float fresnel(float n2, V3 normal, V3 incident, float reflectivity) {
    float r0 = (1.0f - n2) * __builtin_amdgcn_rcpf(1.0f + n2);  // (colour only: the hardware reciprocal)
    r0 *= r0;
    float x = 1.0f + dot(normal, incident);
    float r = r0 + (1.0f - r0) * x * x * x * x * x;
    return (1.0f - reflectivity) * r + reflectivity;
}

// output_shader.frag:246-262
template <int SC, int SETTLE = 0>
__device__ __forceinline__ V3 render_reflection(const FrameConst& F, V3 ro, V3 rd, Tally& cnt) {
    V3 q;
    float dist = cast_ray_d<SC, false>(F, ro, rd, q, cnt);
    if (dist > 0.0f) {
        Mat m;
        V3 p = ro + rd * dist;
        const bool pl = plane_probes<SC>(F, p);
        V3 n = normal_fast<SC>(F, p, cnt, pl);
        return light_O<SC, SETTLE>(F, q, ro, rd, p, n, n, pl, m, cnt);
    }
    return background<ScenePolicy<SC>::kTrim>(ro, rd);
}

// output_shader.frag:298-343 (MAX_REFRACTIONS 4); live only in test scene OG
template <int SC, int SETTLE = 0>
__device__ __forceinline__ V3 render_refraction(const FrameConst& F, V3 ro, V3 rd, V3 absorption, Tally& cnt) {
    V3 color = v3s(0.0f);
    float invert = -1.0f;
    float absorb = 0.0f;
    for (int i = 0; i < 4; i++) {
        V3 q;
        float dist = invert < 0.0f ? cast_ray_d<SC, true>(F, ro, rd, q, cnt) : cast_ray_d<SC, false>(F, ro, rd, q, cnt);
        if (invert < 0.0f) absorb += dist;
        if (dist < 0.0f) {
            if (invert > 0.0f) color = color + background<ScenePolicy<SC>::kTrim>(ro, rd);
            break;
        }
        Mat m;
        V3 p = ro + rd * dist;
        const bool pl = plane_probes<SC>(F, p);
        V3 g = normal_fast<SC>(F, p, cnt, pl);
        V3 n = g * invert;
        V3 ref = reflect(rd, n);
        color = color + light_O<SC, SETTLE>(F, q, ro, ref, p, n, g, pl, m, cnt);
        if (invert > 0.0f) break;
        float ior = invert < 0.0f ? m.refraction_index : 1.0f / m.refraction_index;
        V3 raf = refract(rd, n, ior);
        bool tif = raf.x == 0.0f && raf.y == 0.0f && raf.z == 0.0f;
        rd = tif ? ref : raf;
        ro = p + rd * (0.01f / fabsf(dot(rd, n)));
        invert = tif ? invert : -invert;
    }
    constexpr float kLog2e = 1.4426950408889634f;  // exp(-absorption * absorb), colour only (ScenePolicy)
    return color * v3(__builtin_amdgcn_exp2f(-absorption.x * absorb * kLog2e),
                      __builtin_amdgcn_exp2f(-absorption.y * absorb * kLog2e),
                      __builtin_amdgcn_exp2f(-absorption.z * absorb * kLog2e));
}

// output_shader.frag:348-385 (SETTLE: soft_shadow2's SM)
template <int SC, int SETTLE = 0>
__device__ __forceinline__ V3 render_O(const FrameConst& F, V3 ro, V3 rd, Tally& cnt) {
    V3 q;
    float dist = cast_ray_d<SC, false>(F, ro, rd, q, cnt);
    if (!(dist > 0.0f)) return background<ScenePolicy<SC>::kTrim>(ro, rd);
    Mat m;
    V3 p = ro + rd * dist;
    const bool pl = plane_probes<SC>(F, p);
    V3 n = normal_fast<SC>(F, p, cnt, pl);
    V3 color = light_O<SC, SETTLE>(F, q, ro, rd, p, n, n, pl, m, cnt);
    float rf = fresnel(m.refraction_index, n, rd, m.transparency > 0.0f ? 0.0f : m.reflectivity);
    if (m.reflectivity > 0.0f) {
        V3 r = reflect(rd, n);
        color = color + (render_reflection<SC, SETTLE>(F, p + r * 0.001f, r, cnt) * rf) * m.reflectivity;
    }
    if constexpr (SC == SCENE_OG || SC == SCENE_PLUGIN) {  // (scene O has no transparent material)
        if (m.transparency > 0.0f) {
            V3 r = refract(rd, n, 1.0f / m.refraction_index);
            color = color + (render_refraction<SC, SETTLE>(F, p + r * 0.001f, r, m.absorption, cnt) * (1.0f - rf)) *
                                m.transparency;
        }
    }
    return color;
}

// template.frag:45-76 (scene T); NB: sponge_folds; SETTLE: soft_shadow2_T_loop;
// RSTOP: cast_ray_T's RS for the reflection march, and the far-sky shortcut's mode (below)
// render_T_from: the same with the primary ray's sponge-space image given by the
// caller (rm_shade.h builds it per lane for rays with origins of their own)
template <int NB = 3, int SETTLE = 0, int RSTOP = 0>
__device__ __forceinline__ V3 render_T_from(const FrameConst& F, const LinRay& prim, V3 ro, V3 rd, Tally& cnt) {
    constexpr int SC = SCENE_T;
    using P = ScenePolicy<SC>;
    // The far-sky shortcut (rm_far_sky.h states the proof): in a wave whose active lanes all pass
    // far_sky_ray the primary march returns ZFAR and the reflection factor is 1, on every lane, whatever their
    // steps.  Decided per wave (a scalar branch: a mixed wave marches as before), with RSTOP's modes: 1 (timed
    // kernels) takes neither march, 2 (instrumented) takes both and counts all their steps in cnt.skipped.
    // The near-sky ladder (rm_far_sky.h 3.): the timed kernels take the same vote against the cube
    // of half-size F.near_r, the smallest the launch's step cap admits (the host's choice; never larger than
    // kFarSkyR where F.far_sky is set, and the test is monotonic in r: a far-sky wave passes it).  The instrumented
    // kernels keep cnt.skipped to the far-sky vote and count the marches of the waves that pass the new vote alone
    // in cnt.near_sky, less the reflection steps that cast_ray_T's RS = 2 already put into cnt.skipped.
    bool far = false, vote = false;
    if constexpr (P::kFarSky && RSTOP != 0) {
        if (F.near_r > 0.0f) {
            float r = F.near_r;
            asm volatile("" : "+v"(r));  // (once per wave: an SGPR here and the literal 2^-100 do not fit one FMA)
            vote = __builtin_amdgcn_ballot_w64(
                      rmfs::near_sky_ray(prim.o.x, prim.o.y, prim.o.z, prim.d.x, prim.d.y, prim.d.z, r)) ==
                  __builtin_amdgcn_ballot_w64(true);  // (every active lane)
        }
        if constexpr (RSTOP == 2) {
            if (F.far_sky)
                far = __builtin_amdgcn_ballot_w64(
                          rmfs::far_sky_ray(prim.o.x, prim.o.y, prim.o.z, prim.d.x, prim.d.y, prim.d.z)) ==
                      __builtin_amdgcn_ballot_w64(true);
        } else {
            far = vote;
        }
    }
    const bool near = RSTOP == 2 && vote && !far;
    const uint32_t e0 = cnt.evals;
    float depth = ZFAR;
    if (RSTOP != 1 || !far) depth = cast_ray_T<NB>(F, prim, cnt);
    if constexpr (RSTOP == 2) {
        cnt.skipped += far ? cnt.evals - e0 : 0u;
        cnt.near_sky += near ? cnt.evals - e0 : 0u;
    }
    V3 p = ro + rd * depth;
    // (the timed kernels' far-sky waves: the normal's and the AO's probes as box terms, normal_fast's BOX)
    const bool boxp = RSTOP == 1 && far;
    V3 n;
    if (boxp) n = normal_fast<SC, NB, true>(F, p, cnt);
    else n = normal_fast<SC, NB>(F, p, cnt);
    float c = 1.0f;
    if (RSTOP != 1 || !far) {
        // getColorReflect (common.frag:991-1002); its dead nr normal is skipped
        const uint32_t e1 = cnt.evals, s1 = cnt.skipped;
        V3 rdir = reflect(rd, n);
        V3 ror = p + rdir * 0.01f;
        const LinRay rray = sponge_ray(F, ror, rdir);
        // The reflection certificate (rm_refl_clear.h states the proof): a reflection ray that
        // leaves a face of the sponge's cube outward at a slope >= kRatio meets nothing and passes depth 3 within
        // kSteps steps, so with max_steps >= kSteps (a uniform compare: a smaller cap marches as before) its
        // factor c is exactly 1.0f.  With RSTOP's modes: 1 (timed kernels) such a lane does not march -- a wave
        // whose lanes are all clear leaves the loop's exec mask empty and branches over it, pr, pd and the sqrt;
        // 2 (instrumented) takes the march and counts in cnt.refl_cleared those of its steps that are in neither
        // cnt.skipped (the steps from depth 3 on; every step of a far-sky wave) nor cnt.certified, for the lanes
        // that hit the sponge; 0 marches.
        bool rclear = false;
        if constexpr (P::kReflClear && RSTOP != 0)
            rclear = (F.max_steps >= rmrc::kSteps) &
                     rmrc::refl_clear(rray.o.x, rray.o.y, rray.o.z, rray.d.x, rray.d.y, rray.d.z);
        if (RSTOP != 1 || !rclear) {
            V3 pr = ror + rdir * cast_ray_T<NB, RSTOP>(F, rray, cnt);
            if constexpr (RSTOP == 2) {
                cnt.skipped = far ? s1 + (cnt.evals - e1) : cnt.skipped;
                // counted for the lanes whose primary march ended in a hit (the distance at its last point again,
                // into a tally nobody reads): a sky lane that passes the test marches a step or two from its far
                // point, and those stay uncounted, so that a frame without a hit counts 0 under every step cap
                Tally none;
                const bool phit = menger_at<NB>(prim, depth, none) < 0.001f;
                cnt.refl_cleared += rclear && phit ? (cnt.evals - e1) - (cnt.skipped - s1) : 0u;
                // (a near-sky wave's lanes all end at ZFAR, where phit is false: the two never overlap)
                cnt.near_sky += near ? (cnt.evals - e1) - (cnt.skipped - s1) : 0u;
            }
            // |pr - p| >= 0.01 (the offset of ror; the march adds depth >= ZNEAR along rdir): far above 2^-96, below
            // which alone sqrtf's rescaling acts, so the bare v_sqrt_f32 is length()'s float (apply_scattering, TRIM)
            const V3 pd = pr - p;
            c = clamp01_as<P::kTrim>(__builtin_amdgcn_sqrtf(dot(pd, pd)) * (1.0f / 3.0f));
        }
        (void)e1; (void)s1;
    }
    (void)e0;
    const V3 lightPos = v3(20.0f, 50.0f, 0.0f);
    V3 Ld = lightPos - p;
    float ld2 = dot(Ld, Ld);
    V3 lightDir = Ld * __builtin_amdgcn_rsqf(ld2);
    float occ;
    if (boxp) occ = ao_real<SC, NB, true>(F, p, n, cnt);
    else occ = ao_real<SC, NB>(F, p, n, cnt);
    // The shadow certificate (rm_shadow_clear.h states the proof): a lit lane whose shadow ray
    // leaves a face of the sponge's cube outward at a slope >= kRatio gets exactly 1.0f from the march, whatever
    // its steps.  With RSTOP's modes, as shadow_if_lit's: 1 (timed kernels) such a lane does not march -- the test
    // runs inside the lit branch only, and a wave whose lit lanes are all clear leaves the loop's exec mask empty
    // and branches over it; 2 (instrumented) takes the march and counts in cnt.certified those of its steps that
    // are not in cnt.skipped already (an unlit lane's steps stay in skipped, clear or not, and so do a clear
    // lane's steps after its settle point); 0 marches.
    const LinRay sray = sponge_ray(F, p, lightDir);
    const float smint = 0.01f, smaxt = __builtin_amdgcn_sqrtf(ld2);
    const float dotLN = dot(lightDir, n);
    float sha;
    if constexpr (P::kShadowClear && RSTOP == 1) {
        sha = 1.0f;
        if (!(dotLN < 0.0f)) {
            if (!rmsc::shadow_clear(sray.o.x, sray.o.y, sray.o.z, sray.d.x, sray.d.y, sray.d.z, smint))
                sha = soft_shadow2_T<NB, SETTLE>(F, sray, smint, smaxt, cnt);
        }
    } else {
        const uint32_t e2 = cnt.evals, s2 = cnt.skipped;
        sha = shadow_if_lit<RSTOP>(dotLN, cnt, [&] { return soft_shadow2_T<NB, SETTLE>(F, sray, smint, smaxt, cnt); });
        if constexpr (P::kShadowClear && RSTOP == 2) {
            const bool clear = !(dotLN < 0.0f) &&
                               rmsc::shadow_clear(sray.o.x, sray.o.y, sray.o.z, sray.d.x, sray.d.y, sray.d.z, smint);
            // the march's steps less those it already put into cnt.skipped (the steps after its settle point,
            // SETTLE == 2): what the timed kernels would have executed of it, so the two counts never overlap
            cnt.certified += clear ? (cnt.evals - e2) - (cnt.skipped - s2) : 0u;
        }
        (void)e2; (void)s2;
    }
    // The three clamps as clamp01_as (one v_med3_f32, folded into the clamp modifier of the instruction before
    // it, instead of two compares and two selects each), in the form of DESIGN.md 2.17:
    //   NaN: the median differs from GLSL's clamp only for a NaN argument, and the arguments (finite pos, rd,
    //   lightDir) are NaN only when the normal n is.  Then the AO ray is built from n (sponge_ray(p, n)), every
    //   coordinate of its probes' box term is NaN and occ is NaN; occ multiplies all three terms, and phong of a
    //   NaN normal returns NaN (neither of its `< 0` tests holds): the shading is NaN in both forms.
    //   Signed zero: med3 gives +0 where clamp01 gives -0.  The terms are added to phong's (a sum: the zero's
    //   sign is lost unless every term is a zero), and the shading reaches the pixel only through color * (1 - e)
    //   + fog * e with fog * e > 0 (apply_scattering: e = exp2(..) > 0), where a zero of either sign adds nothing.
    float sky = clamp01_as<P::kTrim>(0.5f + 0.5f * n.y);
    float ind = clamp01_as<P::kTrim>(dot(n, mnormalize<SC>(lightDir * v3(-1.0f, 0.0f, -1.0f))));
    float fre = clamp01_as<P::kTrim>(1.0f + dot(n, rd));
    fre = fre * fre;  // pow(x, 2.0)
    // shadow_pow(1) is (1, 1, 1) exactly (v_log_f32(1) = 0, v_exp_f32(0) = 1), and sha is 1 on every lane that
    // took no shadow march or whose march met nothing: the log2 and the two exp2 only in waves with a shadowed lane
    // (the empty asm keeps it a branch: left free, the compiler computes shadow_pow in every wave and selects)
    V3 spow = v3s(1.0f);
    if (__builtin_amdgcn_ballot_w64(sha != 1.0f) != 0) {
        float s = sha;
        asm volatile("" : "+v"(s));
        spow = shadow_pow(s);
    }
    V3 shading = phong(v3(1.64f, 1.27f, 0.99f), v3(1.0f, 1.0f, 0.0f), 1280.0f, lightDir, p, ro, n) * spow;
    shading = shading + v3(0.16f, 0.20f, 0.28f) * sky * occ;
    shading = shading + v3(0.40f, 0.28f, 0.20f) * ind * occ;
    shading = shading + v3s(fre * occ);
    return apply_scattering<P::kTrim>(v3s(c) * shading, ro, p);
}
template <int NB = 3, int SETTLE = 0, int RSTOP = 0>
__device__ __forceinline__ V3 render_T(const FrameConst& F, V3 ro, V3 rd, Tally& cnt) {
    // ro is the camera, u_pos: its sponge-space image is the frame's, F.camq_* (rm_device.h camera_sponge_origin)
    float qx = F.camq_x, qy = F.camq_y, qz = F.camq_z;
    // (in VGPRs, as the lanes' own results were: an SGPR addend makes the march's three FMAs per step the slow
    // issue form)
    asm volatile("" : "+v"(qx), "+v"(qy), "+v"(qz));
    // sponge_rot's four constants in VGPRs as well, for the pixel's eleven transforms (the normal's four probes,
    // the AO, reflection, shadow and primary rays): the same instructions in the fast issue form; C3 0.3659-0.3678
    // -> 0.3639-0.3653 ms, six alternating runs each.  G is F but for those four members.
    FrameConst G = F;
    asm volatile("" : "+v"(G.ry_c), "+v"(G.ry_s), "+v"(G.rx_c), "+v"(G.rx_s));
    const LinRay prim{v3(qx, qy, qz), sponge_rot<ScenePolicy<SCENE_T>::kExactMarch>(G, rd.x, rd.y, rd.z)};
    return render_T_from<NB, SETTLE, RSTOP>(G, prim, ro, rd, cnt);
}

// BASELINE config-1 scene S0: castRayD + normal + lambert
__device__ __forceinline__ V3 render_S0(const FrameConst& F, V3 ro, V3 rd, Tally& cnt) {
    constexpr int SC = SCENE_S0;
    V3 q;
    float dist = cast_ray_d<SC, false>(F, ro, rd, q, cnt);
    if (dist > 0.0f) {
        V3 p = ro + rd * dist;
        V3 n = normal_fast<SC>(F, p, cnt);
        V3 lightDir = mnormalize<SC>(v3(20.0f, 50.0f, 0.0f) - p);
        return v3(0.2f, 0.02f, 0.02f) * (0.1f + clamp01(dot(n, lightDir)));
    }
    return background<ScenePolicy<SC>::kTrim>(ro, rd);  // (|rd ZFAR|^2 ~ 2500: apply_scattering's TRIM)
}

// Camera (output_shader.frag:388-404): gl_TexCoord at the pixel centre.
// FAST (scenes S0/T): the divisions by the per-frame W, H and u_resolution.y
// as v_rcp + mul, spelled out: left to -freciprocal-math, the compiler hoisted
// a correctly rounded 1/W out of the persistent kernel's tile loop but not out
// of the one-tile kernels, and their frames differed in a pixel.
template <bool FAST>
__device__ __forceinline__ void camera_ray(const FrameConst& F, int x, int y, float& tcx, float& tcy, V3& ro, V3& rd) {
    if constexpr (FAST) {
        // F.rcp_*: the v_rcp_f32 of (float)W, (float)H and res_y, computed on the device once per resolution
        // (rm_render_host.cpp frame_rcp): the floats the three converts and reciprocals gave here in every wave
        tcx = ((float)x + 0.5f + F.jit_x) * F.rcp_w;
        tcy = ((float)y + 0.5f + F.jit_y) * F.rcp_h;
    } else {
        tcx = ((float)x + 0.5f + F.jit_x) / (float)F.W;  // (jitter 0 outside rm_render_accumulate*)
        tcy = ((float)y + 0.5f + F.jit_y) / (float)F.H;
    }
    const float ux = FAST ? (tcx - 0.5f) * F.res_x * F.rcp_res_y : (tcx - 0.5f) * F.res_x / F.res_y;
    const float uy = FAST ? (tcy - 0.5f) * F.res_y * F.rcp_res_y : (tcy - 0.5f) * F.res_y / F.res_y;
    ro = v3(F.pos_x, F.pos_y, F.pos_z);
    if constexpr (FAST) {
        // normalize() = a * (1 / sqrtf(dot)) compiles to the range-guarded sqrt (apply_scattering, TRIM) and a
        // reciprocal of the frexp mantissa rescaled by ldexp (5 VALU), which is v_rcp_f32's float for a normal
        // argument.  dot = ux^2 + uy^2 + 1 lies in [1, 3) for any aspect up to 2:1 (|ux| <= aspect / 2,
        // |uy| <= 1/2) and stays a normal float for any finite aspect: the bare v_sqrt_f32 and v_rcp_f32.
        const V3 v = v3(ux, -uy, -1.0f);
        rd = v * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(dot(v, v)));
    } else {
        rd = normalize(v3(ux, -uy, -1.0f));
    }
    // rd.yz *= rot(-u_mouse.y); rd.xz *= rot(u_mouse.x)  (row vector x mat2(c,-s,s,c))
    float y1 = rd.y * F.cam1_c + rd.z * -F.cam1_s;
    float z1 = rd.y * F.cam1_s + rd.z * F.cam1_c;
    float x2 = rd.x * F.cam2_c + z1 * -F.cam2_s;
    float z2 = rd.x * F.cam2_s + z1 * F.cam2_c;
    rd = v3(x2, y1, z2);
}

// The pixel store of a render launch.  With F.accumulate (progressive
// accumulation, rm_render_accumulate*: the ping-pong u_sample plumbing of
// main.cpp:192-207 and common.frag:8-11, read by the pass) the target holds
// u_sample, this pixel of the previous frame, and receives
// mix(u_sample, colour, u_sample_part) (GLSL mix as the fixture renderer
// evaluates it, x + (y - x) a, no contraction); RGBA8 targets are read as GL
// reads unorm8 texels, b * RN(1/255) (within 1 ulp of b / 255).  A part >= 1
// (the first frame of a still camera) stores the colour: the target needs no
// clearing.
// SAT (scenes S0/T): the RGBA8 word from the saturating packed converts (rm_device.h pack_rgb8_opaque).
template <bool SAT, typename OUT>
__device__ __forceinline__ void store_pixel(const FrameConst& F, OUT* __restrict__ out, size_t i, V3 c) {
#pragma clang fp contract(off)
    if (F.accumulate && F.sample_part < 1.0f) {
        V3 prev;
        if constexpr (sizeof(OUT) == 4) {
            const uint32_t w = out[i];
            const float k = 1.0f / 255.0f;
            prev = v3((float)(w & 255u) * k, (float)((w >> 8) & 255u) * k, (float)((w >> 16) & 255u) * k);
        } else {
            const float4 v = out[i];
            prev = v3(v.x, v.y, v.z);
        }
        const float a = F.sample_part;
        c = v3(prev.x + (c.x - prev.x) * a, prev.y + (c.y - prev.y) * a, prev.z + (c.z - prev.z) * a);
    }
    if constexpr (sizeof(OUT) == 4) out[i] = SAT ? pack_rgb8_opaque(c.x, c.y, c.z) : pack_rgba8(c.x, c.y, c.z, 1.0f);
    else out[i] = make_float4(c.x, c.y, c.z, 1.0f);
}

// local packed row j of this shard -> frame row y
__device__ __forceinline__ int shard_row(const FrameConst& F, int j) {
    int c = div_by(j, F.run_magic, F.run), r = j - c * F.run;
    return c * F.cycle + F.offset + r;
}
// The same for a wave's rows row0 + jw + dl (jw wave-uniform, dl the lane's row in the wave), scenes S0/T
// (ScenePolicy::kTileRow), by F.tile_run (the host's wave_row_mode, rm_rows.h):
//   1  the part is every row of the frame (cycle = run, offset 0): c cycle + r = c run + r = j, no division;
//   2  the wave's rows lie in one run: c is the wave's and r = r(row0 + jw) + dl, so y = shard_row(row0 + jw) + dl
//      in integers -- the division once per wave on the scalar unit (s_mul_hi_u32; the host sets 2 only with a
//      run_magic) instead of v_mul_hi_u32 and v_mul_lo per lane;
//   0  any other layout (a band of 3, ragged parts, a part starting inside a wave's rows): the per-lane form.
// UNIFORM: jw is wave-uniform as the compiler sees it (one-wave workgroups: the workgroup's first row)
template <bool UNIFORM>
__device__ __forceinline__ int shard_row_of_wave(const FrameConst& F, int jw, int dl) {
    if (F.tile_run == 1) return F.row0 + jw + dl;
    if (F.tile_run == 2) {
        const int jb = F.row0 + (UNIFORM ? jw : __builtin_amdgcn_readfirstlane(jw));
        const int c = (int)__umulhi((uint32_t)jb, F.run_magic);
        return c * (F.cycle - F.run) + F.offset + jb + dl;  // c cycle + offset + (jb - c run) + dl
    }
    return shard_row(F, F.row0 + jw + dl);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The frame around a tile's pixels, shared by render_tile_at below and the
// scene plugins' plugin_render_tile (rm_plugin_kernels.h).  (Their
// dispatch-order lookup, tile_order -> (bx, by), is stated in both: as a
// shared function it compiled to other code, a commuted multiply.  Change
// them together.)
// a one-wave tile's duration in shader clocks, for F.tile_cost: the next launch's dispatch order
__device__ __forceinline__ uint32_t tile_clocks(uint64_t t_start) {
    const uint64_t dt = clock64() - t_start;
    return dt > 0xffffffffull ? 0xffffffffu : (uint32_t)dt;
}
// instrumented launches: pixel (x, packed row j)'s ray-steps into the step map,
// the wave's tallies into evals[0..5]
__device__ __forceinline__ void store_tally(const FrameConst& F, unsigned long long* evals, const Tally& cnt, int x,
                                            int j, int lane) {
    if (F.evals_map && x < F.W && j < F.nrows) F.evals_map[(size_t)j * F.W + x] = cnt.evals;
    uint32_t se = wave_sum_u32(cnt.evals), sf = wave_sum_u32(cnt.flop), ss = wave_sum_u32(cnt.skipped);
    uint32_t sc = wave_sum_u32(cnt.certified), sr = wave_sum_u32(cnt.refl_cleared), sn = wave_sum_u32(cnt.near_sky);
    if (lane == 0) {
        atomicAdd(&evals[0], (unsigned long long)se);
        atomicAdd(&evals[1], (unsigned long long)sf);
        if (ss) atomicAdd(&evals[2], (unsigned long long)ss);
        if (sc) atomicAdd(&evals[3], (unsigned long long)sc);
        if (sr) atomicAdd(&evals[4], (unsigned long long)sr);
        if (sn) atomicAdd(&evals[5], (unsigned long long)sn);
    }
}

// SETTLE: the timed kernels' exact early exits (1), which the instrumented
// (COUNT) kernels do not take but count (2): their ray-step counts and maps
// stay the reference's, rm_stats.skipped the steps the timed kernels leave out
template <int SC, int NB = 3, int SETTLE = 0, int RSTOP = 0>
__device__ __forceinline__ V3 render_pixel(const FrameConst& F, V3 ro, V3 rd, Tally& cnt) {
    if constexpr (SC == SCENE_S0) return render_S0(F, ro, rd, cnt);
    else if constexpr (SC == SCENE_T) return render_T<NB, SETTLE, RSTOP>(F, ro, rd, cnt);
    else return render_O<SC, SETTLE>(F, ro, rd, cnt);  // O, OG and plugins: output_shader.frag's render()
}

// sceneSDF(p) of the scene at n points (rm_scene_eval): the distance in the
// reference's arithmetic (the EXACT form), and, when mat is set, the 16 floats
// of struct Material (common.frag:20-35) in declaration order.
//
// FORM (rm_scene_eval_form): kFormExact is the above.  kFormProbe /
// kFormProbeNb1 store scene_dist<SC, kProbeForm> (NB = 3 / 1) instead, where
// dist is set, and into aux, where it is set, the probe form's slack of
// scene_dist_O (the value plane_probes thresholds; 0 for the other scenes).
// The material is scene_mat's in every form, except a plugin's, which comes
// from the instance of the scene library the distance came from.
template <int SC, int FORM = kFormExact>
__device__ __forceinline__ void scene_eval_one(const FrameConst& F, const float* pts, long long n, float* dist,
                                               float* mat, float* aux = nullptr) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 p = v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    Tally t;
    if constexpr (FORM == kFormExact) {
        dist[i] = scene_dist<SC, kExactForm>(F, p, t);
    } else {
        float d, slack = 0.0f;
        // scene O: scene_dist's own call, with its slack (one evaluation gives both)
        if constexpr (SC == SCENE_O || SC == SCENE_OG) d = scene_dist_O<kProbeForm>(p, sponge_space<kProbeForm>(F, p), t, slack);
        else d = scene_dist<SC, kProbeForm, FORM == kFormProbeNb1 ? 1 : 3>(F, p, t);
        if (dist) dist[i] = d;
        if (aux) aux[i] = slack;
    }
    if (mat) {
        Mat m;
        if constexpr (SC == SCENE_PLUGIN && FORM != kFormExact) m = PluginScene<SC>::mat_probe(p);
        else m = scene_mat<SC>(F, p);
        const float v[16] = {m.diffuse.x,    m.diffuse.y,    m.diffuse.z,    m.specular.x,    m.specular.y,  m.specular.z,
                             m.shininess,    m.reflectivity, m.transparency, m.absorption.x,  m.absorption.y,
                             m.absorption.z, m.refraction_index,          m.emission.x,   m.emission.y,    m.emission.z};
        for (int k = 0; k < 16; k++) mat[16 * i + k] = v[k];
    }
}

// Workgroup shapes (KernelKind): KERNEL_TILE16 = 16x16 pixels as 2x2 waves
// of 8x8; KERNEL_TILE8 = one 8x8-pixel wave per workgroup (the dispatcher
// then refills CUs at wave granularity, which shortens the tail of small or
// uneven launches); KERNEL_TILE16X4 = one 16x4-pixel wave.
// KERNEL_PERSIST = 8x8-pixel one-wave tiles pulled by persistent waves from an
// atomic tile counter (SURVEY.md 7.5's refill at tile granularity, rm_params.kernel 4).
enum KernelKind : int { KERNEL_TILE16 = 0, KERNEL_TILE8 = 1, KERNEL_TILE16X4 = 2, KERNEL_PERSIST = 3 };
template <int K> struct Tiling;
template <> struct Tiling<KERNEL_TILE16> { static constexpr int TW = 16, TH = 16, WPB = 4, LW = 8; };
template <> struct Tiling<KERNEL_TILE8> { static constexpr int TW = 8, TH = 8, WPB = 1, LW = 8; };
template <> struct Tiling<KERNEL_TILE16X4> { static constexpr int TW = 16, TH = 4, WPB = 1, LW = 16; };
template <> struct Tiling<KERNEL_PERSIST> : Tiling<KERNEL_TILE8> {};

// The body of a render launch: one lane per pixel of the workgroup's tile.
// OUT = float4 (gl_FragColor) or uint32_t (RGBA8, packed in the epilogue, so
// the displayed frame costs 4 B/px of HBM instead of 16 + 20 for a pack
// pass).  COUNT: instrumented build, ray-steps and FLOP summed per wave into
// evals[0..5] (ray-steps, FLOP, ray-steps the timed kernels skip by an early exit, by the shadow certificate, by
// the reflection certificate, and by the near-sky ladder).
// (bx, by): the tile's position in dispatch order on a gx-wide tile grid
// (blockIdx for the hardware-dispatched kernels).
template <int SC, bool COUNT, int K, typename OUT>
__device__ __forceinline__ void render_tile_at(const FrameConst& F, OUT* __restrict__ out,
                                               unsigned long long* __restrict__ evals, int bx, int by, int gx) {
    using T = Tiling<K>;
    using P = ScenePolicy<SC>;
    const uint64_t t_start = T::WPB == 1 && F.tile_cost ? clock64() : 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // scene T: the first lat_tiles workgroups of an ordered launch are its
    // costliest tiles, whose lone waves end the launch; they render with one
    // fold exit test instead of three (fewer branches, more VALU: C4 share and
    // C2 tails -16..19 %, a whole C3 frame +5 % if every tile did)
    const bool lat = T::WPB == 1 && SC == SCENE_T && F.tile_order && by * gx + bx < F.lat_tiles;
    if (F.tile_order) {  // dispatch order != tile order (costliest tiles first, rm_set_tile_order)
        const uint32_t t = F.tile_order[by * gx + bx];
        by = div_by((int)t, F.gx_magic, gx);
        bx = (int)t - by * gx;
    }
    const int x = bx * T::TW + (w & 1) * 8 + (lane % T::LW);
    const int j = by * T::TH + (w >> 1) * 8 + (lane / T::LW);
    // OUT = WireTile (rm_render_cycle_rows_wire): the wave's 8x8 tile is not
    // stored as pixels but encoded for the compressed wire from registers
    // (rm_wire_tile.h) into the workspace, tile by * gx + bx of the part
    constexpr bool kWire = IsWireTile<OUT>::value;
    static_assert(!kWire || (T::WPB == 1 && T::TW == 8 && T::TH == 8), "the wire codes one 8x8 wave tile");
    uint32_t wire_px = 0;  // (kWire: this lane's RGBA8 word, 0 outside the part)
    Tally cnt;
    if (x < F.W && j < F.nrows) {
        int y;
        if constexpr (P::kTileRow)  // (one-wave workgroups: w = 0, the wave's first row is the workgroup's)
            y = shard_row_of_wave<T::WPB == 1>(F, by * T::TH + (T::WPB == 1 ? 0 : (w >> 1) * 8), lane / T::LW);
        else y = shard_row(F, F.row0 + j);
        float tcx, tcy;
        V3 ro, rd;
        camera_ray<P::kHwMath>(F, x, y, tcx, tcy, ro, rd);
        const float vig = vignette(tcx, tcy);
        V3 c;
        if constexpr (SC == SCENE_T) {
            // (no settle exit in the latency tiles: their long grazing shadow marches
            // settle late or never, and the test lengthens the lone waves that end
            // the launch: C4 share +16 %, C2 P1 +12 % with it)
            if (lat) c = render_pixel<SC, 1, 0, COUNT ? 2 : 1>(F, ro, rd, cnt);
            else c = render_pixel<SC, 3, COUNT ? 2 : 1, COUNT ? 2 : 1>(F, ro, rd, cnt);
        } else {
            (void)lat;
            c = render_pixel<SC, 3, P::kSettleO ? (COUNT ? 2 : 1) : 0>(F, ro, rd, cnt);
        }
        c = post_colour<P::kTrim>(c, vig);
        if constexpr (kWire) wire_px = P::kTrim ? pack_rgb8_opaque(c.x, c.y, c.z) : pack_rgba8(c.x, c.y, c.z, 1.0f);
        else store_pixel<P::kTrim>(F, out, (size_t)j * F.W + x, c);
    }
    if constexpr (kWire)
        wire_encode_tile(wire_px, reinterpret_cast<WireTile*>(out), (long long)gx * ((F.nrows + 7) / 8),
                         (long long)by * gx + bx);
    if (T::WPB == 1 && F.tile_cost && lane == 0) F.tile_cost[by * gx + bx] = tile_clocks(t_start);
    if constexpr (COUNT) store_tally(F, evals, cnt, x, j, lane);
}

template <int SC, bool COUNT, int K, typename OUT>
__device__ __forceinline__ void render_tile(const FrameConst& F, OUT* __restrict__ out,
                                            unsigned long long* __restrict__ evals) {
    render_tile_at<SC, COUNT, K, OUT>(F, out, evals, blockIdx.x, blockIdx.y, gridDim.x);
}

// Persistent waves (KERNEL_PERSIST): the dispatch ordinals k of the launch's
// tiles are dealt to the 8 XCDs (k = x + 8 j on XCD x = blockIdx.x % 8, the
// dispatcher's round robin), each XCD's waves pulling j from a counter of
// their own (F.persist[kPersistStride * x]: device-scope atomics on one address
// from all XCDs serialize), the next j fetched before the current tile renders
// (the atomic's latency hides behind the tile).  Tile k renders as the
// hardware-dispatched kernel renders workgroup k (same tile order, latency
// tiles, tile durations), so pixels are identical.  The last wave to leave
// (counter 8 counts them) resets the counters for the next launch that uses
// them; no wave waits for another.
constexpr int kPersistStride = 32;  // uint32 words between counters (128 B lines)
constexpr int kPersistWords = 9 * kPersistStride;
template <int SC, bool COUNT, typename OUT>
__device__ __forceinline__ void render_persistent(const FrameConst& F, OUT* __restrict__ out,
                                                  unsigned long long* __restrict__ evals, int gx, int ntiles) {
    const int xcd = blockIdx.x & 7;
    uint32_t* ctr = F.persist + kPersistStride * xcd;
    const int nj = (ntiles - xcd + 7) >> 3;  // ordinals xcd, xcd + 8, ... below ntiles
    auto ticket = [&]() {
        int j = 0;
        if (threadIdx.x == 0) j = (int)atomicAdd(ctr, 1u);
        return __builtin_amdgcn_readfirstlane(j);
    };
    for (int j = ticket(); j < nj;) {
        const int jn = ticket();
        const int k = xcd + 8 * j;
        const int ky = div_by((int)k, F.gx_magic, gx);
        render_tile_at<SC, COUNT, KERNEL_PERSIST, OUT>(F, out, evals, (int)k - ky * gx, ky, gx);
        j = jn;
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(F.persist + 8 * kPersistStride, 1u) == gridDim.x - 1)
            for (int x = 0; x < 9; x++) atomicExch(F.persist + kPersistStride * x, 0u);
    }
}

}  // namespace rm
