// near_sky_test.cpp -- scene T's near-sky ladder (csrc/rm_far_sky.h 3.) on the CPU.
// Stand-alone: tests/test_near_sky_host.py builds it with the host compiler under
// the address and undefined-behaviour sanitizers; it includes the predicate's
// header and nothing else of the project.
//
// It restates what the shortcut replaces, in plain C with one rounding per
// operation, as tests/host/far_sky_test.cpp does: cast_ray_T's loop
// (rm_render_direct.h) over mengersponge in the exact form and in the fast form
// the kernels march with, and over the sponge's box term alone -- the least
// distance the proof's premise (dist >= box) allows, where the folds lend no
// help -- and the first step of the RS = 1 reflection march.
// For every rung (m, r, N) of rmfs::kNearSkyLadder and every ray that
// rmfs::near_sky_ray's miss test accepts at r, with |d| in [kUnitLo, kUnitHi]:
// the march meets nothing, every step is >= m, and it returns the bits of ZFAR
// within N steps -- so under the caps N, N + 1, 256 and 512 alike, which a
// subset runs one by one.  The rung choice (rmfs::near_sky_radius) is held to
// the ladder at N - 1 and N of every rung, and every ray accepted at the radius
// chosen for a step cap must return ZFAR under that cap.  The longest march seen
// per rung is printed beside N(m): the proven bound has slack, and the test
// claims no tightness.
//
// Two perturbed builds must fail (tests/test_near_sky_host.py):
//   -DNEAR_SKY_TEST_M=0.01f   the last rung tests the cube of m = 0.01 under the N of m = 0.02
//   -DNEAR_SKY_TEST_NO_CAP    the radius is the last rung's whatever the step cap
// Exits non-zero at the first failed check, naming it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../raymarching_amd/csrc/rm_far_sky.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s (line %d): %s\n", __func__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static const float ZNEAR = 0.02f, ZFAR = 50.0f;
static const int kRungs = rmfs::kNearSkyRungs;

struct Rung {
    float m, r;
    int n;
};
// the ladder under test: the header's, or the first perturbation's
static Rung rung(int i) {
    Rung g{rmfs::kNearSkyLadder[i].m, rmfs::kNearSkyLadder[i].r, rmfs::kNearSkyLadder[i].n};
#ifdef NEAR_SKY_TEST_M
    if (i == kRungs - 1) {
        g.m = NEAR_SKY_TEST_M;
        g.r = 1.0f + g.m + 0x1p-10f;  // (its N stays the header's last)
    }
#endif
    return g;
}
// the radius a launch with this step cap tests: the header's choice, or the second perturbation's
static float radius_for(int max_steps) {
#ifdef NEAR_SKY_TEST_NO_CAP
    (void)max_steps;
    return rmfs::kNearSkyLadder[kRungs - 1].r;
#else
    return rmfs::near_sky_radius(max_steps, true);
#endif
}

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
// form: kFast / kExact (mengersponge as the kernels march it), or kBox: the box term alone, the smallest distance the
// proof allows (dist >= box is all it uses of the scene), which is what the step bound has to hold for
enum { kFast = 0, kExact = 1, kBox = 2, kForms = 3 };
static float box_term(V3 p) { return std::fmax(std::fabs(p.x), std::fmax(std::fabs(p.y), std::fabs(p.z))) - 1.0f; }
static float cast_ray(const Ray &s, int max_steps, int form, float &min_dist, int &steps) {
    float depth = ZNEAR;
    min_dist = std::numeric_limits<float>::infinity();
    steps = 0;
    for (int i = 0; i < max_steps; i++) {
        const float dist = form == kBox ? box_term(at(s, depth)) : menger(at(s, depth), form == kExact);
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

static bool miss(const Ray &s, float r) { return rmfs::ray_misses_cube(s.o.x, s.o.y, s.o.z, s.d.x, s.d.y, s.d.z, r); }
static bool far_clear(const Ray &s) { return rmfs::far_point_clear(s.o.x, s.o.y, s.o.z, s.d.x, s.d.y, s.d.z); }
static bool unit_range(V3 d) {  // the |d| the ladder is offered to
    const double l = std::sqrt((double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z);
    return l >= rmfs::kUnitLo && l <= rmfs::kUnitHi;
}
static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof(u));
    return u;
}

static long g_accepted[8], g_band[8], g_caps[8], g_reflect[8];
static int g_longest[8], g_longest_box[8];

// the claims for one world ray (ro, rd) under rotation R on rung i; returns whether the miss test accepted it.
// (A direction outside the unit range is the host's to keep away, rm_render_host.cpp: the march is not checked.)
static bool check_prim(int i, const Rot &R, V3 ro, V3 rd, const Ray &prim, bool all_caps) {
    const Rung g = rung(i);
    const bool acc = miss(prim, g.r);
    CHECK(rmfs::near_sky_ray(prim.o.x, prim.o.y, prim.o.z, prim.d.x, prim.d.y, prim.d.z, g.r) == (acc && far_clear(prim)));
    // the ladder is nested: what a wider rung accepts, this one does
    if (i > 0 && miss(prim, rung(i - 1).r)) CHECK(acc);
    if (!acc || !unit_range(prim.d)) return acc;
    g_accepted[i]++;
    if (!miss(prim, rmfs::kFarSkyR)) g_band[i]++;
    for (int form = 0; form < kForms; form++) {
        float min_dist;
        int steps;
        const float depth = cast_ray(prim, 512, form, min_dist, steps);
        CHECK(bits(depth) == bits(ZFAR));
        CHECK(!(min_dist < 0.001f));
        CHECK(min_dist >= g.m);  // the step bound's own premise
        CHECK(steps <= g.n);     // so every cap >= N(m) gives the same march
        int &longest = form == kBox ? g_longest_box[i] : g_longest[i];
        if (steps > longest) longest = steps;
        if (all_caps) {
            for (int cap : {g.n, g.n + 1, 256, 512}) {
                float md;
                int st;
                CHECK(bits(cast_ray(prim, cap, form, md, st)) == bits(ZFAR));
                CHECK(st == steps && !(md < 0.001f));
            }
            if (form == kExact) g_caps[i]++;
        }
    }
    if (all_caps && far_clear(prim)) {  // condition 2 needs the far point alone
        g_reflect[i]++;
        Rng rn{(uint64_t)g_reflect[i]};
        CHECK(reflection_factor(R, ro, rd, rn.dir(), false) == 1.0f);
        CHECK(reflection_factor(R, ro, rd, rn.dir(), true) == 1.0f);
    }
    return true;
}
static bool check_ray(int i, const Rot &R, V3 ro, V3 rd, bool all_caps) {
    return check_prim(i, R, ro, rd, sponge_ray(R, ro, rd), all_caps);
}
// a ray given in sponge space, bit for bit (the world origin, which only the reflection's far point uses, is its
// image under the identity rotation, rounded)
static bool check_sponge_ray(int i, V3 o, V3 d, bool all_caps = true) {
    return check_prim(i, kIdentity, V3{o.x, o.y + 3.0f, o.z}, d, Ray{o, d}, all_caps);
}

static V3 axes(int k, float a, float b, float c) {  // (a, b, c) rolled so that a lands on axis k
    float v[3];
    v[k] = a;
    v[(k + 1) % 3] = b;
    v[(k + 2) % 3] = c;
    return V3{v[0], v[1], v[2]};
}

static void random_rays(int i) {
    const Rung g = rung(i);
    Rng rng{20261020ull + (uint64_t)i};
    const long n = 1000000;
    long acc = 0;
    for (long j = 0; j < n; j++) {
        V3 o, d;
        const int kind = (int)(j & 3);
        if (kind == 0) {  // sponge-space origins in [-8, 8]^3, unit directions
            o = V3{rng.uni(-8.0f, 8.0f), rng.uni(-8.0f, 8.0f), rng.uni(-8.0f, 8.0f)};
            d = rng.dir();
        } else {
            // through a point within [-0.003, 0.03] of the tested cube's surface, nearly along the face (kind 1),
            // across an edge (2) or freely (3), from 0.2 to 9 units before it or (every 16th) from up to 900
            const int k = (int)(rng.next() % 3);
            const float s = (rng.next() & 1) ? 1.0f : -1.0f, off = g.r + rng.uni(-0.003f, 0.03f);
            V3 p = axes(k, s * off, rng.uni(-off, off), rng.uni(-off, off));
            if (kind == 2) p = axes(k, s * off, ((rng.next() & 1) ? off : -off), rng.uni(-off, off));
            if (kind == 1) d = unit(axes(k, s * rng.uni(-0.002f, 0.02f), rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f)));
            else if (kind == 2) d = unit(axes(k, s * rng.uni(0.0f, 1.0f), rng.uni(-1.0f, 1.0f), rng.uni(-0.3f, 0.3f)));
            else d = rng.dir();
            const float back = (j & 15) == 3 ? rng.uni(9.0f, 900.0f) : rng.uni(0.2f, 9.0f);
            o = add(p, mul(d, -back));
        }
        if ((j & 63) == 5) d = mul(d, (j & 64) ? 0.9991f : 1.0009f);  // both ends of the admitted |d|
        acc += check_sponge_ray(i, o, d, (j & 63) == 0) ? 1 : 0;
    }
    CHECK(acc > n / 4 && acc < n);
    // rotated sponges (u_time) and world origins near the quoted poses
    for (long j = 0; j < 100000; j++) {
        const float ay = rng.uni(-3.2f, 3.2f), ax = rng.uni(-3.2f, 3.2f);
        const Rot R{std::cos(ay), std::sin(ay), std::cos(ax), std::sin(ax)};
        const V3 ro{rng.uni(-4.0f, 4.0f), rng.uni(-1.0f, 7.0f), rng.uni(-4.0f, 4.0f)};
        check_ray(i, R, ro, rng.dir(), (j & 63) == 0);
    }
    (void)g;
}

static void directed_rays(int i) {
    const Rung g = rung(i);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float den = 1.0e-40f, tiny = std::numeric_limits<float>::denorm_min();
    const float m1 = 1.0f + g.m, up = std::nextafterf(g.r, 2.0f);
    const float sg[2] = {1.0f, -1.0f};
    // parallel to a face at exactly 1 + m and the adjacent floats (inside the slack: refused), at r itself (the
    // comparison is strict: refused) and at the next float above r (taken: the slowest ray of the rung), on
    // every axis and side, along both other axes, from 7 and from 1000 units before the cube
    for (int k = 0; k < 3; k++)
        for (float s : sg)
            for (float off : {std::nextafterf(m1, 0.0f), m1, std::nextafterf(m1, 2.0f), g.r, up, g.r + 0x1p-9f})
                for (int j = 1; j < 3; j++)
                    for (float back : {7.0f, 1000.0f}) {
                        float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
                        o[k] = s * off;
                        o[(k + j) % 3] = -back;
                        o[(k + 3 - j) % 3] = 0.3f;
                        d[(k + j) % 3] = 1.0f;
                        const bool acc = check_sponge_ray(i, V3{o[0], o[1], o[2]}, V3{d[0], d[1], d[2]});
                        CHECK(acc == (off > g.r));
                    }
    // parallel to a face along its diagonal, corner to corner of the inflated square, 2^-12 inside and outside r:
    // the longest stretch a ray can stay at a distance of m, 2 sqrt2 (1 + m), and the slowest ray this test knows
    for (int k = 0; k < 3; k++)
        for (float s : sg)
            for (float sd : sg)
                for (float off : {g.r - 0x1p-12f, g.r + 0x1p-12f, g.r + 0x1p-9f})
                    for (float back : {0.5f, 5.0f, 500.0f}) {
                        const float h = 0.70710678f, c = off + back;  // (through the square's centre line)
                        CHECK(check_sponge_ray(i, axes(k, s * off, -c, -sd * c), axes(k, 0.0f, h, sd * h)) == (off > g.r));
                    }
    // along the inflated cube's edges and past its corners: through a point just inside / outside them
    for (float e : {g.r - 0x1p-12f, up, g.r + 0x1p-9f, g.r + 0.01f})
        for (float sx : sg)
            for (float sy : sg) {
                // along the edge x = y = e, beside it
                CHECK(check_sponge_ray(i, V3{sx * e, sy * e, -6.0f}, V3{0.0f, 0.0f, 1.0f}) == (e > g.r));
                CHECK(check_sponge_ray(i, V3{sx * e, -1000.0f, sy * e}, V3{0.0f, 1.0f, 0.0f}) == (e > g.r));
                // past the edge (direction across it, along z too)
                const V3 through{sx * e, sy * e, 0.1f};
                const V3 d = unit(V3{sx * 1.0f, -sy * 1.0f, 0.3f});
                const bool acc = check_sponge_ray(i, add(through, mul(d, -6.0f)), d);
                if (e < g.r) CHECK(!acc);
                if (e >= g.r + 0x1p-9f) CHECK(acc);
                for (float sz : sg) {  // past the corner, perpendicular to its diagonal
                    const V3 c{sx * e, sy * e, sz * e};
                    const V3 dc = unit(V3{sx * 1.0f, sy * 1.0f, -2.0f * sz});
                    const bool ac = check_sponge_ray(i, add(c, mul(dc, -5.0f)), dc);
                    if (e < g.r) CHECK(!ac);
                    if (e >= g.r + 0x1p-9f) CHECK(ac);
                }
            }
    // zero and denormal direction components, both signs, outside and inside the slab
    for (float z : {0.0f, -0.0f, den, -den, tiny, -tiny})
        for (float s : sg)
            for (float off : {m1 - 0x1p-12f, up, 3.0f}) {
                CHECK(check_sponge_ray(i, V3{s * off, -6.0f, 0.2f}, V3{z, 1.0f, 0.0f}) == (off > g.r));
                CHECK(check_sponge_ray(i, V3{s * off, 0.1f, -6.0f}, V3{z, z, 1.0f}) == (off > g.r));
                CHECK(check_sponge_ray(i, V3{-6.0f, s * off, s * off}, V3{1.0f, z, -z}) == (off > g.r));
            }
    // a zero direction is accepted outside the cube (the predicate asks nothing of |d|) and refused inside
    CHECK(miss(Ray{V3{4.0f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}}, g.r));
    CHECK(!miss(Ray{V3{1.01f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}}, g.r));
    // both ends of the admitted |d|, along a face 2^-12 outside r: the bound's worst direction
    for (float len : {0.99901f, 1.00099f})
        for (float back : {0.5f, 7.0f, 1000.0f})
            CHECK(check_sponge_ray(i, V3{g.r + 0x1p-12f, -back, 0.3f}, V3{0.0f, len, 0.0f}));
    // origins on and inside the inflated cube (of half-size h = r - 2^-12, inside the test's slack: at r itself the
    // cross terms' roundings may go either way): never accepted
    Rng rng{7};
    const float h = g.r - 0x1p-12f;
    CHECK(h > m1);
    for (int j = 0; j < 20000; j++) {
        V3 o{rng.uni(-h, h), rng.uni(-h, h), rng.uni(-h, h)};
        if (j % 4 == 1) o.x = (j & 4) ? h : -h;              // on a face
        if (j % 4 == 2) o.x = o.y = (j & 4) ? h : -h;        // on an edge
        if (j % 4 == 3) o.x = o.y = o.z = (j & 4) ? h : -h;  // at a corner
        CHECK(!check_sponge_ray(i, o, rng.dir(), false));
    }
    // origins 1000 units away: aimed at the sponge (refused), just past the tested cube (taken)
    for (int j = 0; j < 4000; j++) {
        const int k = j % 3;
        const V3 o = axes(k, (j & 4) ? 1000.0f : -1000.0f, rng.uni(-8.0f, 8.0f), rng.uni(-8.0f, 8.0f));
        const V3 target{rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f)};
        CHECK(!check_sponge_ray(i, o, unit(add(target, mul(o, -1.0f)))));
        const float off = g.r + rng.uni(0.002f, 0.05f);
        const V3 beside = axes((k + 1) % 3, (j & 8) ? off : -off, rng.uni(-1.0f, 1.0f), 0.0f);
        check_sponge_ray(i, o, unit(add(beside, mul(o, -1.0f))));
    }
    // non-finite input: refused, whichever component; origins past the range and huge directions too
    for (float bad : {inf, -inf, nan})
        for (int k = 0; k < 6; k++) {
            float v[6] = {3.0f, 0.5f, -0.25f, 1.0f, 0.0f, 0.0f};  // (accepted when finite)
            CHECK(rmfs::near_sky_ray(v[0], v[1], v[2], v[3], v[4], v[5], g.r));
            v[k] = bad;
            CHECK(!rmfs::ray_misses_cube(v[0], v[1], v[2], v[3], v[4], v[5], g.r));
            CHECK(!rmfs::near_sky_ray(v[0], v[1], v[2], v[3], v[4], v[5], g.r));
        }
    CHECK(!rmfs::near_sky_ray(3.0f, 0.5f, -0.25f, 1.0f, 0.0f, 0.0f, nan));  // (and a NaN radius)
    CHECK(!rmfs::near_sky_ray(3.0f, 0.5f, -0.25f, 1.0f, 0.0f, 0.0f, inf));
    CHECK(!rmfs::near_sky_ray(2000.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, g.r));
    CHECK(!rmfs::near_sky_ray(3.0f, 0.0f, 0.0f, 1.0e30f, 0.0f, 0.0f, g.r));
}

// the ladder and the rung choice, in the header's own terms
static void ladder() {
    CHECK(kRungs == 4 && rmfs::kNearSkyLadder[0].r == rmfs::kFarSkyR);
    for (int i = 0; i < kRungs; i++) {
        const rmfs::NearSkyRung &g = rmfs::kNearSkyLadder[i];
        CHECK(g.r == 1.0f + g.m + 0x1p-10f && g.n == rmfs::near_sky_bound(g.r));
        CHECK(g.n >= 1 && g.n <= 256 && g.m >= 0.02f);
        if (i > 0) CHECK(g.r < rmfs::kNearSkyLadder[i - 1].r && g.n > rmfs::kNearSkyLadder[i - 1].n);
        // N - 1 steps: the rung before (or none); N steps: this rung
        CHECK(rmfs::near_sky_radius(g.n - 1, true) == (i > 0 ? rmfs::kNearSkyLadder[i - 1].r : 0.0f));
        CHECK(rmfs::near_sky_radius(g.n, true) == g.r);
    }
    CHECK(rmfs::kNearSkyLadder[2].n <= 128 && rmfs::kNearSkyLadder[3].n <= rmfs::kFarSkyN0);
    for (int cap : {-5, 0, 1, 38}) CHECK(rmfs::near_sky_radius(cap, true) == 0.0f);
    CHECK(rmfs::near_sky_radius(1 << 30, true) == rmfs::kNearSkyLadder[kRungs - 1].r);
    // without unit directions: the far-sky cube from N0 steps on, whose proof asks nothing of |d|
    CHECK(rmfs::near_sky_radius(rmfs::kFarSkyN0 - 1, false) == 0.0f && rmfs::near_sky_radius(rmfs::kFarSkyN0, false) == rmfs::kFarSkyR);
    // a bound for a margin the proof does not cover is no bound
    CHECK(rmfs::near_sky_bound(1.0f + 0.01f + 0x1p-10f) > 1000000 && rmfs::near_sky_bound(std::numeric_limits<float>::quiet_NaN()) > 1000000);
    CHECK(rmfs::unit_rotation(1.0f, 0.0f) && rmfs::unit_rotation(std::cos(0.7f), std::sin(0.7f)));
    CHECK(!rmfs::unit_rotation(0.0f, 0.0f) && !rmfs::unit_rotation(1.0f, 0.02f) && !rmfs::unit_rotation(0.99f, 0.0f));
    CHECK(!rmfs::unit_rotation(std::numeric_limits<float>::quiet_NaN(), 0.0f) &&
          !rmfs::unit_rotation(std::numeric_limits<float>::infinity(), 0.0f));
}

// every ray accepted at the radius chosen for a step cap returns ZFAR under that cap
static void caps() {
    Rng rng{99};
    long marched = 0;
    for (int i = 0; i < kRungs; i++)
        for (int cap : {rmfs::kNearSkyLadder[i].n - 1, rmfs::kNearSkyLadder[i].n, 128, 207, 208, 256}) {
            const float r = radius_for(cap);
            if (!(r > 0.0f)) continue;
            const float up = std::nextafterf(r, 2.0f);
            for (int j = 0; j < 400; j++) {
                Ray s;
                if (j < 8) s = Ray{axes(j % 3, up, -(float)(1 << j), 0.3f), axes(j % 3, 0.0f, 1.0f, 0.0f)};  // along a face
                else {
                    const float off = r + rng.uni(0.0f, 0.01f);
                    const V3 p = axes(j % 3, off, rng.uni(-off, off), rng.uni(-off, off));
                    const V3 d = unit(axes(j % 3, rng.uni(0.0f, 0.01f), rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f)));
                    s = Ray{add(p, mul(d, -rng.uni(0.2f, 9.0f))), d};
                }
                if (!miss(s, r)) continue;
                for (int form = 0; form < kForms; form++) {
                    float md;
                    int st;
                    CHECK(bits(cast_ray(s, cap, form, md, st)) == bits(ZFAR));
                }
                marched++;
            }
        }
    CHECK(marched > 2000);
}

// near_sky_test --eval in.bin out.bin: n records of 7 floats (ox oy oz dx dy dz r, sponge space) -> n bytes of
// rmfs::near_sky_ray; near_sky_test --radius in.bin out.bin: n records of 2 int32 (max_steps, unit_dirs) -> n floats
// of rmfs::near_sky_radius.  For tests/test_near_sky_host.py to hold tests/near_sky_ref.py to.
static int eval_file(const char *in_path, const char *out_path, bool radius) {
    std::FILE *in = std::fopen(in_path, "rb");
    if (!in) {
        std::fprintf(stderr, "near_sky_test: cannot read %s\n", in_path);
        return 2;
    }
    std::FILE *out = std::fopen(out_path, "wb");
    if (!out) {
        std::fprintf(stderr, "near_sky_test: cannot write %s\n", out_path);
        std::fclose(in);
        return 2;
    }
    long n = 0;
    int rc = 0;
    for (;;) {
        float v[7];
        int32_t q[2];
        const size_t want = radius ? 2 : 7;
        const size_t got = radius ? std::fread(q, sizeof(int32_t), 2, in) : std::fread(v, sizeof(float), 7, in);
        if (got == 0) break;
        if (got != want) {
            std::fprintf(stderr, "near_sky_test: %s is not a whole number of records\n", in_path);
            rc = 2;
            break;
        }
        size_t put;
        if (radius) {
            const float r = rmfs::near_sky_radius(q[0], q[1] != 0);
            put = std::fwrite(&r, sizeof(float), 1, out);
        } else {
            const unsigned char b = rmfs::near_sky_ray(v[0], v[1], v[2], v[3], v[4], v[5], v[6]) ? 1 : 0;
            put = std::fwrite(&b, 1, 1, out);
        }
        if (put != 1) {
            std::fprintf(stderr, "near_sky_test: short write to %s\n", out_path);
            rc = 2;
            break;
        }
        n++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) rc = 2;
    if (rc == 0) std::printf("evaluated %ld records\n", n);
    return rc;
}

int main(int argc, char **argv) {
    if (argc == 4 && std::strcmp(argv[1], "--eval") == 0) return eval_file(argv[2], argv[3], false);
    if (argc == 4 && std::strcmp(argv[1], "--radius") == 0) return eval_file(argv[2], argv[3], true);
    if (argc == 2 && std::strcmp(argv[1], "--ladder") == 0) {
        for (int i = 0; i < kRungs; i++)
            std::printf("%.9g %.9g %d\n", (double)rmfs::kNearSkyLadder[i].m, (double)rmfs::kNearSkyLadder[i].r, rmfs::kNearSkyLadder[i].n);
        return 0;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: near_sky_test [--eval in.bin out.bin | --radius in.bin out.bin | --ladder]\n");
        return 2;
    }
    ladder();
    caps();
    for (int i = 0; i < kRungs; i++) {
        directed_rays(i);
        random_rays(i);
        const Rung g = rung(i);
        std::printf("rung m = %g (r = %.9g): %ld accepted rays marched (%ld of them inside the far-sky cube's margin), "
                    "%ld under all four caps, %ld reflection factors; longest march %d steps over the sponge's distance, %d over "
                    "its box term alone, proven N(m) = %d (slack %d: the bound is not tight)\n",
                    (double)g.m, (double)g.r, g_accepted[i], g_band[i], g_caps[i], g_reflect[i], g_longest[i],
                    g_longest_box[i], g.n, g.n - g_longest_box[i]);
    }
    std::printf("all checks passed\n");
    return 0;
}
