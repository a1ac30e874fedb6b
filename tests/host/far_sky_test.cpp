// far_sky_test.cpp -- scene T's far-sky shortcut (csrc/rm_far_sky.h) on the CPU.
// Stand-alone: tests/test_far_sky_host.py builds it with the host compiler under
// the address and undefined-behaviour sanitizers; it includes the predicate's
// header and nothing else of the project.
//
// It restates what the shortcut replaces, in plain C with one rounding per
// operation: cast_ray_T's loop (rm_render_direct.h) over mengersponge
// (rm_device.h sponge_box + sponge_folds, in the exact form and in the fast form
// the kernels march with; no fold exit, which changes no value), the primary
// ray's sponge-space image (sponge_space<false>, sponge_rot<false>) and the
// first step of the RS = 1 reflection march with the colour factor it feeds.
// For every ray the predicate accepts, the march with max_steps = N0 must return
// exactly ZFAR without ever seeing dist < 0.001, in both forms; when the
// far-point condition holds too, the reflection factor must be exactly 1 for
// the point's own gradient normal and for arbitrary unit normals.  Exits
// non-zero at the first failed check, naming it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <utility>

#include "../../raymarching_amd/csrc/rm_far_sky.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s (line %d): %s\n", __func__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static const float ZNEAR = 0.02f, ZFAR = 50.0f;
static const float M = rmfs::kFarSkyM;
static const int N0 = rmfs::kFarSkyN0;

struct V3 {
    float x, y, z;
};
struct Ray {
    V3 o, d;
};
struct Rot {  // FrameConst's ry_c, ry_s, rx_c, rx_s
    float yc, ys, xc, xs;
};
static const Rot kIdentity = {1.0f, 0.0f, 1.0f, 0.0f};

static float med3(float a, float b, float c) { return std::fmax(std::fmin(a, b), std::fmin(std::fmax(a, b), c)); }

// mengersponge(p).x: sdBox's Chebyshev term, then three folds
static float menger(V3 p, bool exact) {
    static const float SH[3] = {0.5f, 1.5f, 4.5f}, S3[3] = {3.0f, 9.0f, 27.0f};
    static const float INV[3] = {1.0f / 3.0f, 1.0f / 9.0f, 1.0f / 27.0f};
    float d = std::fmax(std::fabs(p.x), std::fmax(std::fabs(p.y), std::fabs(p.z))) - 1.0f;
    const float box = d;
    for (int m = 0; m < 3; m++) {
        float r[3];
        const float c3[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; k++) {
            if (exact) {
                const float h = c3[k] * SH[m];
                const float fr = h - floorf(h);
                const float a = fmaf(2.0f, fr, -1.0f);
                const float t = 3.0f * std::fabs(a);
                r[k] = std::fabs(1.0f - t);
            } else {
                const float y = fmaf(c3[k], SH[m], -0.5f);
                const float g = y - rintf(y);
                r[k] = std::fabs(fmaf(-6.0f, std::fabs(g), 1.0f));
            }
        }
        const float med = med3(r[0], r[1], r[2]);
        float c;
        if (exact) {  // div_const(med - 1, s, 1 / s)
            const float x = med - 1.0f, q = x * INV[m];
            const float rem = fmaf(-S3[m], q, x);
            c = fmaf(rem, INV[m], q);
        } else {
            c = fmaf(med, INV[m], -INV[m]);
        }
        d = std::fmax(c, d);
    }
    CHECK(d >= box);  // "the result is >= d": what the proof rests on
    return d;
}

static V3 at(const Ray &r, float t) { return V3{fmaf(r.d.x, t, r.o.x), fmaf(r.d.y, t, r.o.y), fmaf(r.d.z, t, r.o.z)}; }

// cast_ray_T with RS = 0; min_dist: the smallest distance any step saw
static float cast_ray(const Ray &s, int max_steps, bool exact, float &min_dist, int &steps) {
    float depth = ZNEAR;
    min_dist = std::numeric_limits<float>::infinity();
    steps = 0;
    for (int i = 0; i < max_steps; i++) {
        const float dist = menger(at(s, depth), exact);
        steps++;
        min_dist = std::fmin(min_dist, dist);
        const bool hit = dist < 0.001f;
        depth = hit ? depth : depth + dist;
        if (hit || depth >= ZFAR) break;
    }
    return depth >= ZFAR ? ZFAR : depth;
}

// sponge_rot<false> / sponge_space<false>
static V3 rot(const Rot &R, V3 v) {
    const float x1 = fmaf(v.x, R.yc, v.z * R.ys);
    const float z1 = fmaf(v.z, R.yc, -(v.x * R.ys));
    const float y2 = fmaf(v.y, R.xc, -(z1 * R.xs));
    const float z2 = fmaf(z1, R.xc, v.y * R.xs);
    return V3{x1, y2, z2};
}
static Ray sponge_ray(const Rot &R, V3 ro, V3 rd) { return Ray{rot(R, V3{ro.x, ro.y - 3.0f, ro.z}), rot(R, rd)}; }

static float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 mul(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
static V3 unit(V3 a) { return mul(a, 1.0f / std::sqrt(dot(a, a))); }

// the reflection block of render_T_from at the far point p = ro + rd ZFAR with
// normal n, its march cut to the first step as RS = 1 cuts it: the factor c
static float reflection_factor(const Rot &R, V3 ro, V3 rd, V3 n, bool exact) {
    const V3 p = add(ro, mul(rd, ZFAR));
    const V3 rdir = add(rd, mul(n, -(2.0f * dot(n, rd))));  // reflect(rd, n)
    const V3 ror = add(p, mul(rdir, 0.01f));
    const Ray s = sponge_ray(R, ror, rdir);
    float depth = ZNEAR;
    const float dist = menger(at(s, depth), exact);
    CHECK(!(dist < 0.001f));
    depth = depth + dist;
    CHECK(depth >= 3.0f);  // RS = 1 leaves here
    const V3 pr = add(ror, mul(rdir, depth >= ZFAR ? ZFAR : depth));
    const V3 pd = V3{pr.x - p.x, pr.y - p.y, pr.z - p.z};
    const float c = std::sqrt(dot(pd, pd)) * (1.0f / 3.0f);
    return c < 0.0f ? 0.0f : c > 1.0f ? 1.0f : c;
}

// getNormalFast at p (tetrahedral gradient, h = 0.001) in the kernel's fast form
static V3 normal_at(const Rot &R, V3 p) {
    const float h = 0.001f;
    const V3 k[4] = {{h, -h, -h}, {-h, -h, h}, {-h, h, -h}, {h, h, h}};
    V3 g{0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 4; i++) {
        const V3 q = add(p, k[i]);
        const float d = menger(rot(R, V3{q.x, q.y - 3.0f, q.z}), false);
        g = add(g, mul(k[i], d * 1000.0f));
    }
    return unit(g);
}

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
    V3 dir() {
        for (;;) {
            const V3 v{uni(-1.0f, 1.0f), uni(-1.0f, 1.0f), uni(-1.0f, 1.0f)};
            const float l2 = dot(v, v);
            if (l2 > 0.01f && l2 <= 1.0f) return unit(v);
        }
    }
};

static bool miss(const Ray &s) {
    return rmfs::ray_misses_cube(s.o.x, s.o.y, s.o.z, s.d.x, s.d.y, s.d.z, rmfs::kFarSkyR);
}
static bool far_clear(const Ray &s) { return rmfs::far_point_clear(s.o.x, s.o.y, s.o.z, s.d.x, s.d.y, s.d.z); }

static long g_accepted = 0, g_reflect = 0, g_max_steps_seen = 0;

// the two claims for one world ray (ro, rd) under rotation R; returns whether the miss test accepted it
static bool check_ray(const Rot &R, V3 ro, V3 rd, Rng *rng) {
    const Ray prim = sponge_ray(R, ro, rd);
    const bool acc = miss(prim);
    CHECK(rmfs::far_sky_ray(prim.o.x, prim.o.y, prim.o.z, prim.d.x, prim.d.y, prim.d.z) == (acc && far_clear(prim)));
    if (!acc) return false;
    g_accepted++;
    for (int exact = 0; exact < 2; exact++) {
        float min_dist;
        int steps;
        const float depth = cast_ray(prim, N0, exact != 0, min_dist, steps);
        CHECK(depth == ZFAR);
        CHECK(!(min_dist < 0.001f));
        CHECK(min_dist >= M);  // the step bound's own premise
        if (steps > g_max_steps_seen) g_max_steps_seen = steps;
    }
    const float l2 = dot(rd, rd);
    if (far_clear(prim) && std::fabs(l2 - 1.0f) <= 1.0e-4f) {  // (unit rays: shade_ray_ok's guard, camera_ray)
        g_reflect++;
        const V3 p = add(ro, mul(rd, ZFAR));
        CHECK(reflection_factor(R, ro, rd, normal_at(R, p), false) == 1.0f);
        CHECK(reflection_factor(R, ro, rd, normal_at(R, p), true) == 1.0f);
        if (rng) CHECK(reflection_factor(R, ro, rd, rng->dir(), false) == 1.0f);
    }
    return true;
}
// a ray given in sponge space (identity rotation: the image is the ray itself, shifted by the sponge's centre)
static bool check_sponge_ray(V3 o, V3 d, Rng *rng = nullptr) { return check_ray(kIdentity, V3{o.x, o.y + 3.0f, o.z}, d, rng); }

// exact slab test in double against the cube of half-size r, t >= 0
static bool slab_miss(const Ray &s, double r) {
    double t0 = 0.0, t1 = std::numeric_limits<double>::infinity();
    const double o[3] = {s.o.x, s.o.y, s.o.z}, d[3] = {s.d.x, s.d.y, s.d.z};
    for (int k = 0; k < 3; k++) {
        if (d[k] == 0.0) {
            if (std::fabs(o[k]) > r) return true;
            continue;
        }
        double a = (-r - o[k]) / d[k], b = (r - o[k]) / d[k];
        if (a > b) std::swap(a, b);
        t0 = std::fmax(t0, a);
        t1 = std::fmin(t1, b);
    }
    return t0 > t1;
}

static void random_rays() {
    Rng rng{20240601};
    long pred = 0, slab = 0;
    const long n = 1000000;
    for (long i = 0; i < n; i++) {  // sponge-space origins in [-8, 8]^3, unit directions
        const V3 o{rng.uni(-8.0f, 8.0f), rng.uni(-8.0f, 8.0f), rng.uni(-8.0f, 8.0f)};
        const V3 d = rng.dir();
        const bool acc = check_sponge_ray(o, d, (i & 15) == 0 ? &rng : nullptr);
        const Ray prim = sponge_ray(kIdentity, V3{o.x, o.y + 3.0f, o.z}, d);
        const bool ref = slab_miss(prim, 1.0 + (double)M + 0.01);
        pred += acc ? 1 : 0;
        slab += ref ? 1 : 0;
        CHECK(acc || !ref);   // not vacuous, ray by ray: 0.01 of room holds every rounding
        CHECK(slab_miss(prim, 1.0 + (double)M) || !acc);  // and never more than the exact test at 1 + m
    }
    CHECK(pred >= slab && slab > n / 2);
    std::printf("random rays: %ld of %ld accepted (exact slab test at 1 + m + 0.01: %ld)\n", pred, n, slab);
    // rotated sponges (u_time) and world origins near the quoted poses
    for (long i = 0; i < 200000; i++) {
        const float ay = rng.uni(-3.2f, 3.2f), ax = rng.uni(-3.2f, 3.2f);
        const Rot R{std::cos(ay), std::sin(ay), std::cos(ax), std::sin(ax)};
        const V3 ro{rng.uni(-8.0f, 8.0f), rng.uni(-5.0f, 11.0f), rng.uni(-8.0f, 8.0f)};
        check_ray(R, ro, rng.dir(), (i & 15) == 0 ? &rng : nullptr);
    }
}

static void directed_rays() {
    const float m1 = 1.0f + M, e = 0x1p-12f, inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN(), den = 1.0e-40f, tiny = std::numeric_limits<float>::denorm_min();
    const float sg[2] = {1.0f, -1.0f};
    // parallel to a face at offsets 1 + m +- 2^-12, on every axis and side, along both other axes
    for (int k = 0; k < 3; k++)
        for (float s : sg)
            for (float off : {m1 - e, m1, m1 + e, m1 + 2.0f * e, m1 + 0x1p-9f})
                for (int j = 1; j < 3; j++) {
                    float o[3] = {-7.0f, 0.3f, -0.2f}, d[3] = {0.0f, 0.0f, 0.0f};
                    o[k] = s * off;
                    o[(k + j) % 3] = -7.0f;
                    o[(k + 3 - j) % 3] = 0.3f;
                    d[(k + j) % 3] = 1.0f;
                    const bool acc = check_sponge_ray(V3{o[0], o[1], o[2]}, V3{d[0], d[1], d[2]});
                    CHECK(acc == (off >= m1 + 0x1p-9f));  // inside the slack: refused; 2^-9 out: taken
                }
    // grazing the inflated cube's edges and corners: through a point just inside / outside them
    for (float g : {m1 - e, m1 + e, m1 + 0x1p-9f, m1 + 0.01f})
        for (float sx : sg)
            for (float sy : sg) {
                // past the edge x = y = g (direction across it, along z too)
                const V3 through{sx * g, sy * g, 0.1f};
                const V3 d = unit(V3{sx * 1.0f, -sy * 1.0f, 0.3f});
                const V3 o = add(through, mul(d, -6.0f));
                const bool acc = check_sponge_ray(o, d);
                CHECK(acc == (g >= m1 + 0x1p-9f));
                for (float sz : sg) {  // past the corner, perpendicular to its diagonal
                    const V3 c{sx * g, sy * g, sz * g};
                    const V3 dc = unit(V3{sx * 1.0f, sy * 1.0f, -2.0f * sz});
                    const bool ac = check_sponge_ray(add(c, mul(dc, -5.0f)), dc);
                    CHECK(ac == (g >= m1 + 0x1p-9f));
                }
            }
    // zero and denormal direction components, both signs, outside and inside the slab
    for (float z : {0.0f, -0.0f, den, -den, tiny, -tiny})
        for (float s : sg)
            for (float off : {m1 - e, m1 + 0x1p-9f, 3.0f}) {
                CHECK(check_sponge_ray(V3{s * off, -6.0f, 0.2f}, V3{z, 1.0f, 0.0f}) == (off > m1));
                CHECK(check_sponge_ray(V3{s * off, 0.1f, -6.0f}, V3{z, z, 1.0f}) == (off > m1));
                CHECK(check_sponge_ray(V3{-6.0f, s * off, s * off}, V3{1.0f, z, -z}) == (off > m1));
            }
    CHECK(check_sponge_ray(V3{4.0f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}));   // a zero direction marches in place, outside
    CHECK(!check_sponge_ray(V3{1.2f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}));  // and inside the inflated cube
    // origins on and inside the inflated cube: never accepted
    Rng rng{7};
    for (int i = 0; i < 20000; i++) {
        V3 o{rng.uni(-m1, m1), rng.uni(-m1, m1), rng.uni(-m1, m1)};
        if (i % 4 == 1) o.x = (i & 4) ? m1 : -m1;  // on a face
        if (i % 4 == 2) o.x = o.y = (i & 4) ? m1 : -m1;  // on an edge
        if (i % 4 == 3) o.x = o.y = o.z = (i & 4) ? m1 : -m1;  // at a corner
        CHECK(!check_sponge_ray(o, rng.dir()));
    }
    // the camera inside the inflated cube but outside the sponge (world (0, 3, 1.2))
    for (int i = 0; i < 2000; i++) CHECK(!check_ray(kIdentity, V3{0.0f, 3.0f, 1.2f}, rng.dir(), nullptr));
    // origins 60 units away: aimed at the sponge (refused), past it (taken; far points near the sponge fail the second condition)
    long near_far = 0;
    for (int i = 0; i < 20000; i++) {
        const V3 o = mul(rng.dir(), 60.0f);
        const V3 target{rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f)};
        CHECK(!check_sponge_ray(o, unit(add(target, mul(o, -1.0f)))));
        const V3 beside = mul(rng.dir(), rng.uni(1.3f, 6.0f));
        check_sponge_ray(o, unit(add(beside, mul(o, -1.0f))));
        // from 50.5 to 53 units the far point, at depth ZFAR, lands beside the sponge
        const V3 o2 = mul(rng.dir(), rng.uni(50.5f, 53.0f));
        const V3 d2 = unit(add(beside, mul(o2, -1.0f)));
        const Ray s{o2, d2};
        if (check_sponge_ray(o2, d2) && !far_clear(s)) near_far++;
    }
    CHECK(near_far > 100);  // accepted by the miss test, far point within 4.1: the reflection keeps its march
    // non-finite input: refused, whichever component
    for (float bad : {inf, -inf, nan})
        for (int k = 0; k < 6; k++) {
            float v[6] = {3.0f, 0.5f, -0.25f, 1.0f, 0.0f, 0.0f};  // (accepted when finite)
            CHECK(rmfs::far_sky_ray(v[0], v[1], v[2], v[3], v[4], v[5]));
            v[k] = bad;
            CHECK(!rmfs::ray_misses_cube(v[0], v[1], v[2], v[3], v[4], v[5], rmfs::kFarSkyR));
            CHECK(!rmfs::far_sky_ray(v[0], v[1], v[2], v[3], v[4], v[5]));
            for (int j = 0; j < 6; j++) {  // and with a second one
                float w[6] = {3.0f, 0.5f, -0.25f, 1.0f, 0.0f, 0.0f};
                w[k] = bad;
                w[j] = j == k ? bad : -inf;
                CHECK(!rmfs::far_sky_ray(w[0], w[1], w[2], w[3], w[4], w[5]));
            }
        }
    // origins past the predicate's range and huge directions: refused
    CHECK(!rmfs::far_sky_ray(2000.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f));
    CHECK(!rmfs::far_sky_ray(3.0f, 0.0f, 0.0f, 1.0e30f, 0.0f, 0.0f));
    CHECK(!rmfs::far_sky_ray(3.0e38f, 3.0e38f, 3.0e38f, 1.0f, 0.0f, 0.0f));
}

static void step_bound() {
    // N0 (0.25 - 2^-19) + ZNEAR reaches ZFAR, in the proof's own arithmetic
    CHECK((double)ZNEAR + (double)N0 * ((double)M - 0x1p-19) >= (double)ZFAR);
    CHECK(rmfs::kFarSkyR == 1.0f + M + 0x1p-10f && (double)rmfs::kFarSkyR == 1.0 + (double)M + 0x1p-10);
    CHECK(rmfs::kFarSkyDepth == ZFAR);
}

// far_sky_test --eval in.bin out.bin: n rays of 6 floats (ox oy oz dx dy dz, sponge space) -> n bytes of
// rmfs::far_sky_ray, for tests/test_far_sky_host.py to hold tests/far_sky_ref.py's numpy restatement to
static int eval_file(const char *in_path, const char *out_path) {
    std::FILE *in = std::fopen(in_path, "rb");
    if (!in) {
        std::fprintf(stderr, "far_sky_test: cannot read %s\n", in_path);
        return 2;
    }
    std::FILE *out = std::fopen(out_path, "wb");
    if (!out) {
        std::fprintf(stderr, "far_sky_test: cannot write %s\n", out_path);
        std::fclose(in);
        return 2;
    }
    float v[6];
    long n = 0, accepted = 0;
    int rc = 0;
    for (;;) {
        const size_t got = std::fread(v, sizeof(float), 6, in);
        if (got == 0) break;
        if (got != 6) {
            std::fprintf(stderr, "far_sky_test: %s is not a whole number of rays\n", in_path);
            rc = 2;
            break;
        }
        const unsigned char b = rmfs::far_sky_ray(v[0], v[1], v[2], v[3], v[4], v[5]) ? 1 : 0;
        if (std::fwrite(&b, 1, 1, out) != 1) {
            std::fprintf(stderr, "far_sky_test: short write to %s\n", out_path);
            rc = 2;
            break;
        }
        n++;
        accepted += b;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) rc = 2;
    if (rc == 0) std::printf("evaluated %ld rays, %ld far-sky\n", n, accepted);
    return rc;
}

int main(int argc, char **argv) {
    if (argc == 4 && std::strcmp(argv[1], "--eval") == 0) return eval_file(argv[2], argv[3]);
    if (argc != 1) {
        std::fprintf(stderr, "usage: far_sky_test [--eval in.bin out.bin]\n");
        return 2;
    }
    step_bound();
    directed_rays();
    random_rays();
    std::printf("accepted rays marched: %ld, reflection factors checked: %ld, longest escaping march: %ld steps (N0 = %d)\n",
                g_accepted, g_reflect, g_max_steps_seen, N0);
    std::printf("all checks passed\n");
    return 0;
}
