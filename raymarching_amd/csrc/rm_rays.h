// rm_rays.h -- ray queries (rm_cast_rays, rm_camera_rays): castRayD / castRayDI
// (common.frag:879-925) over caller-supplied rays, one lane per ray, and the
// rays main() builds for a frame (output_shader.frag:388-405).
//
// The march here is the GLSL's plain loop over the scene's exact-form distance.
// It takes none of the render kernels' shortcuts (floor-plane spans,
// sponge-space rays, settle exits, hardware-math forms, rm_render_direct.h):
// those rest on unit camera rays and on what a frame needs, and a query's rd
// is used as given.  Built-in scenes are instantiated in rm_rays.hip, a scene
// plugin's in its own translation unit (rm_plugin_kernels.h rm_plugin_cast).
//
// Layout: origins and directions are tightly packed xyz triples, read as three
// dwords per lane at stride 12 B: the three loads of a wave cover the same 768
// contiguous bytes, every 128-B line of them fully used, so the triples are not
// staged through LDS (the march is VALU-bound: DESIGN.md 2.19).  Outputs are
// struct-of-arrays: t, status and steps are coalesced dword stores.
// Nothing indexes memory by ray data, and every loop is bounded by max_steps:
// non-finite rays leave by the same exits (a NaN distance fails both tests and
// marches to the step cap).
#pragma once
#include "rm_render_direct.h"

#include "rm_libm_ref.h"

namespace rm {

enum : int { RAY_MISS = 0, RAY_HIT = 1, RAY_EXHAUSTED = 2 };  // include/rm.h RM_RAY_*

// One launch's rays and outputs (device pointers).  Outputs left null are not
// written; normal and material are wave-uniform "is it wanted" flags as well,
// so a distance-only query pays for neither.
struct RayQuery {
    const float* origins;     // n xyz triples, or one shared by every ray (shared_origin)
    const float* directions;  // n xyz triples
    long long n;
    int shared_origin;
    float* t;                   // n
    int* status;                // n
    uint32_t* steps;            // n
    float* position;            // n x 3
    float* normal;              // n x 3
    float* material;            // n x 16
    unsigned long long* evals;  // [0] += the launch's steps (rm_stats.evals), or null
};

// getNormalFast (common.frag:697-708) over the exact-form distance with the
// GLSL's normalize: normal_fast<SC>'s arithmetic for scenes O, OG and plugins;
// scenes S0/T, whose render kernels use the hardware forms there, get the
// exact forms too (a query is not a frame)
template <int SC>
__device__ __forceinline__ V3 ray_normal(const FrameConst& F, V3 p) {
    const float h = 0.001f;
    Tally scratch;  // (normal taps are not steps of the march)
    const float d0 = scene_dist<SC, kExactForm>(F, p + v3(h, -h, -h), scratch);
    const float d1 = scene_dist<SC, kExactForm>(F, p + v3(-h, -h, h), scratch);
    const float d2 = scene_dist<SC, kExactForm>(F, p + v3(-h, h, -h), scratch);
    const float d3 = scene_dist<SC, kExactForm>(F, p + v3(h, h, h), scratch);
    V3 g = v3(d0, -d0, -d0) + v3(-d1, -d1, d1);
    g = g + v3(-d2, d2, -d2);
    g = g + v3(d3, d3, d3);
    return normalize(g);
}

// floorMat (output_shader.frag:16-28) in the CPU restatement's arithmetic: the
// GLSL's operations one by one, sin and pow as the C library evaluates them
// (rm_libm_ref.h).  floor_mat (rm_device.h), the render kernels' form, is
// within 6e-6 of it; a query's caller compares materials, so it gets this one.
__device__ __forceinline__ Mat floor_mat_ref(V3 pos) {
    const float scale = gmax(10.0f, libm::pow_ref(length(pos), 1.3f));
    const float tx = smoothstep<false>(-0.005f, 0.005f, libm::sin_ref(pos.x * PI_REF) / scale);
    const float ty = smoothstep<false>(-0.005f, 0.005f, libm::sin_ref(pos.z * PI_REF) / scale);
    const float tile = gmin(gmax(tx, ty), gmax(1.0f - tx, 1.0f - ty));
    return Mat(mix3(v3s(0.3f), v3s(0.025f), tile), v3s(0.03f), 128.0f, 0.0f, 0.0f, v3s(0.0f), 1.0f, v3s(0.0f));
}

// The material half of sceneSDF at p: scene_mat<SC> (rm_device.h), with scene
// O's floor from floor_mat_ref.  (Scene O's blend is scene_mat's, restated
// around the other floor; change them together.)
template <int SC>
__device__ __forceinline__ Mat ray_mat(const FrameConst& F, V3 p) {
    if constexpr (SC == SCENE_O || SC == SCENE_OG) {
        uint32_t fl = 0;
        const float d0 = menger<kExactForm>(sponge_space<kExactForm>(F, p), fl);
        const float d1 = len3<kExactForm, false>(p.x - 3.0f, p.y - 2.0f, p.z - 3.0f) - 1.0f;
        const float d2 = cube<kExactForm>(p, v3(-5.0f, 4.0f, 5.0f), 1.0f);
        const float d3 = p.y;
        float m1, m2, m3;
        const float t1 = smin_cubic_d<kExactForm>(d1, d2, 0.5f, m1);
        const Mat b = mat_blue(SC == SCENE_OG);
        const Mat mt1 = smin_mat(d1, b, d2, b, m1);
        const float t2 = smin_cubic_d<kExactForm>(t1, d3, 0.5f, m2);
        const Mat mt2 = smin_mat(t1, mt1, d3, floor_mat_ref(p), m2);
        (void)smin_cubic_d<kExactForm>(d0, t2, 0.33f, m3);
        return smin_mat(d0, mat_mirror(), t2, mt2, m3);
    } else {
        return scene_mat<SC>(F, p);
    }
}

struct RayHit {
    float t;         // castRayD's dist: the depth on a hit, -1 past ZFAR, the last distance when max_steps ran out
    int status;      // RAY_*
    uint32_t steps;  // sceneSDF calls of the march
    V3 last;         // the last point evaluated (ro without steps): the point of the SdResult castRayD returns
};

// common.frag:879-901 (INSIDE: castRayDI, :903-925; depth -= d is depth + (-d), the same float)
template <int SC, bool INSIDE>
__device__ __forceinline__ RayHit cast_one(const FrameConst& F, V3 ro, V3 rd) {
    RayHit h{0.0f, RAY_EXHAUSTED, 0u, ro};
    float depth = ZNEAR;
    Tally scratch;
    for (int i = 0; i < F.max_steps; i++) {
        const V3 q = ro + rd * depth;
        const float res = scene_dist<SC, kExactForm>(F, q, scratch);
        const float d = INSIDE ? -res : res;
        h.last = q;
        h.steps++;
        h.t = res;
        if (d < 0.001f * depth) {
            h.t = depth;
            h.status = RAY_HIT;
            break;
        }
        depth = depth + d;
        if (depth >= ZFAR) {
            h.t = -1.0f;
            h.status = RAY_MISS;
            break;
        }
    }
    return h;
}

// The body of a cast launch: ray i = blockIdx.x * blockDim.x + threadIdx.x.
template <int SC>
__device__ __forceinline__ void cast_rays_one(const FrameConst& F, const RayQuery& Q, int inside) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t steps = 0;
    if (i < Q.n) {
        const float* o = Q.shared_origin ? Q.origins : Q.origins + 3 * i;
        const V3 ro = v3(o[0], o[1], o[2]);
        const V3 rd = v3(Q.directions[3 * i], Q.directions[3 * i + 1], Q.directions[3 * i + 2]);
        const RayHit h = inside ? cast_one<SC, true>(F, ro, rd) : cast_one<SC, false>(F, ro, rd);  // (wave-uniform)
        steps = h.steps;
        Q.t[i] = h.t;
        if (Q.status) Q.status[i] = h.status;
        if (Q.steps) Q.steps[i] = h.steps;
        // the point render() shades (output_shader.frag:351-355): where dist > 0
        const bool shade = h.t > 0.0f;
        const V3 p = ro + rd * h.t;
        if (Q.position) {
            Q.position[3 * i] = shade ? p.x : 0.0f;
            Q.position[3 * i + 1] = shade ? p.y : 0.0f;
            Q.position[3 * i + 2] = shade ? p.z : 0.0f;
        }
        if (Q.normal) {
            V3 n = v3s(0.0f);
            if (shade) n = ray_normal<SC>(F, p);
            Q.normal[3 * i] = n.x;
            Q.normal[3 * i + 1] = n.y;
            Q.normal[3 * i + 2] = n.z;
        }
        if (Q.material) {
            const Mat m = ray_mat<SC>(F, h.last);
            const float v[16] = {m.diffuse.x,    m.diffuse.y,    m.diffuse.z,    m.specular.x,    m.specular.y,  m.specular.z,
                                 m.shininess,    m.reflectivity, m.transparency, m.absorption.x,  m.absorption.y,
                                 m.absorption.z, m.refraction_index,          m.emission.x,   m.emission.y,    m.emission.z};
            for (int k = 0; k < 16; k++) Q.material[16 * i + k] = v[k];
        }
    }
    if (Q.evals) {  // (wave-uniform; every lane of the wave arrives here)
        const uint32_t s = wave_sum_u32(steps);
        if ((threadIdx.x & 63) == 0) atomicAdd(&Q.evals[0], (unsigned long long)s);
    }
}

// main()'s rays for the W x H frame (F.W, F.H; no jitter): u_pos into origin3
// (when not null), pixel (x, y)'s direction into directions[3 (y W + x)], row 0
// first.  FAST: the camera_ray form of the loaded scene's render kernel
// (ScenePolicy::kHwMath).
template <bool FAST>
__device__ __forceinline__ void camera_rays_one(const FrameConst& F, float* origin3, float* directions) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && origin3) {
        origin3[0] = F.pos_x;
        origin3[1] = F.pos_y;
        origin3[2] = F.pos_z;
    }
    if (i >= (long long)F.W * F.H) return;
    const int y = (int)(i / F.W), x = (int)(i - (long long)y * F.W);
    float tcx, tcy;
    V3 ro, rd;
    camera_ray<FAST>(F, x, y, tcx, tcy, ro, rd);
    directions[3 * i] = rd.x;
    directions[3 * i + 1] = rd.y;
    directions[3 * i + 2] = rd.z;
}

#ifndef __HIPCC_RTC__
// rm_rays.hip: the built-in scenes' cast kernel and the camera-ray kernel
hipError_t launch_cast_rays(int scene, const FrameConst& F, const RayQuery& Q, int inside, hipStream_t s);
hipError_t launch_camera_rays(bool fast, const FrameConst& F, float* origin3, float* directions, hipStream_t s);
// threads per workgroup of a cast launch
int cast_block_size();
#endif

}  // namespace rm
