// shadow_clear_test.cpp -- scene T's soft-shadow certificate (csrc/rm_shadow_clear.h) on the CPU.
// Stand-alone: tests/test_shadow_clear_host.py builds it with the host compiler
// under the address and undefined-behaviour sanitizers; it includes the
// predicate's header and nothing else of the project.
//
// It restates what the certificate replaces, in plain C with one rounding per
// operation: soft_shadow2_T_loop (rm_render_direct.h) in its num/den form over
// mengersponge (rm_device.h sponge_box + sponge_folds, in the exact form and in
// the fast form the kernels march with; no fold exit, which changes no value),
// without a step cap and capped at 1, 2 and 7 steps, with and without the
// settle exit of the timed kernels.  For every ray the predicate accepts, every
// one of these marches must return the bits of 1.0f, must never update num/den
// and must never see h below kRatio * mint.  Exits non-zero at the first failed
// check, naming it.  (Built with -DRM_SHADOW_CLEAR_RATIO=0.2f it must fail:
// the header's proof does not carry there.)
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../raymarching_amd/csrc/rm_shadow_clear.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s (line %d): %s\n", __func__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static const float K = rmsc::kRatio;
static const float MINT = 0.01f;  // render_T_from's mint

struct V3 {
    float x, y, z;
};
struct Ray {
    V3 o, d;
};

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

struct March {
    float res;      // the returned shadow factor
    float min_h;    // the smallest distance a step saw (inf: no step)
    int updates;    // candidate updates of num/den
    int steps;
};

// soft_shadow2_T_loop: cap = INT_MAX is the uncapped loop copy; settle = the timed kernels' SM = 1
static March soft_shadow(const Ray &s, float mint, float maxt, bool exact, int cap, bool settle) {
    const float kSettleK = (2.9f / 1.01f) * (2.9f / 1.01f) / 16.0f;
    float num = 1.0f / 16.0f, den = 1.0f, P = 0.0f, h = 1.0f;
    float t = mint;
    March m{0.0f, std::numeric_limits<float>::infinity(), 0, 0};
    for (int it = 1; it == 1 ? t < maxt : true; it++) {
        const V3 q = at(s, t);
        const float ax = std::fabs(q.x), ay = std::fabs(q.y), mx = std::fmax(ax, std::fmax(ay, std::fabs(q.z)));
        const float box = mx - 1.0f;
        h = menger(q, exact);
        m.steps++;
        m.min_h = std::fmin(m.min_h, h);
        const float h2 = h * h;
        const float Q = it == 1 ? 1.0f : fmaf(P, P, -h2);
        const float D = it == 1 ? t : fmaf(t, P, -h2);
        const bool away = h + h >= P;
        const float cn = h2 * Q, cd = D * std::fabs(D);
        const bool upd = (Q >= 0.0f) && (cn * den < num * cd);
        num = upd ? cn : num;
        den = upd ? cd : den;
        m.updates += upd ? 1 : 0;
        if (settle && box >= 0.1f && away) {
            const float sx = q.x < 0.0f ? -s.d.x : s.d.x, sy = q.y < 0.0f ? -s.d.y : s.d.y;
            const float sz = q.z < 0.0f ? -s.d.z : s.d.z;
            const float sl = ax == mx ? sx : ay == mx ? sy : sz;
            const float be = fmaf(sl, maxt - t, box);
            if ((sl >= 0.0f) && (kSettleK * box * box * den >= num * t * t) &&
                (kSettleK * be * be * den >= num * maxt * maxt))
                break;
        }
        P = h + h;
        t = fmaf(h, 0.1f, t + 0.001f);
        if ((h < 0.001f) || !(t < maxt)) break;
        if (cap != INT_MAX && it >= cap) break;
    }
    m.res = h < 0.001f ? 0.0f : std::sqrt(16.0f * num * (1.0f / den));
    return m;
}

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static bool clear(const Ray &s, float mint = MINT) {
    return rmsc::shadow_clear(s.o.x, s.o.y, s.o.z, s.d.x, s.d.y, s.d.z, mint);
}

static long g_accepted = 0, g_marches = 0, g_longest = 0;
static float g_min_ratio = std::numeric_limits<float>::infinity();

// the claim for one sponge-space ray; returns whether the predicate accepted it.  `full`: every loop variant
// (else the exact form's long uncapped marches are left out; the capped ones and the fast form always run)
static bool check_ray(const Ray &s, float maxt, bool full = true, float mint = MINT) {
    if (!clear(s, mint)) return false;
    g_accepted++;
    for (int exact = 0; exact < 2; exact++)
        for (int cap : {INT_MAX, 1, 2, 7})
            for (int settle = 0; settle < 2; settle++) {
                if (!full && exact && cap == INT_MAX) continue;
                const March m = soft_shadow(s, mint, maxt, exact != 0, cap, settle != 0);
                g_marches++;
                CHECK(bits(m.res) == bits(1.0f));
                CHECK(m.updates == 0);
                CHECK(m.steps == 0 || m.min_h >= K * mint * 0.999f);  // the bound's own premise
                if (m.steps > g_longest) g_longest = m.steps;
                if (m.steps > 0 && cap == INT_MAX && !settle && !exact) g_min_ratio = std::fmin(g_min_ratio, m.min_h / mint);
            }
    return true;
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
            const float l2 = v.x * v.x + v.y * v.y + v.z * v.z;
            if (l2 > 0.01f && l2 <= 1.0f) {
                const float r = 1.0f / std::sqrt(l2);
                return V3{v.x * r, v.y * r, v.z * r};
            }
        }
    }
};

// permute / mirror a ray given for the face x = +1 onto face f = 0..5
static Ray on_face(Ray r, int f) {
    const float sg = (f & 1) ? -1.0f : 1.0f;
    r.o.x *= sg;
    r.d.x *= sg;
    const int ax = f >> 1;
    if (ax == 1) return Ray{V3{r.o.y, r.o.x, r.o.z}, V3{r.d.y, r.d.x, r.d.z}};
    if (ax == 2) return Ray{V3{r.o.z, r.o.y, r.o.x}, V3{r.d.z, r.d.y, r.d.x}};
    return r;
}

static void random_rays() {
    Rng rng{20241020};
    long n_face = 0, acc_face = 0, one_face = 0, acc_of_one = 0, acc_hole = 0, acc_far = 0;
    // origins on a face (offsets of +-0.002: a hit point lies within the march's tolerance of it), over the
    // solid part and over the holes alike, directions leaving it at slopes on both sides of kRatio
    const long n1 = 700000;
    for (long i = 0; i < n1; i++) {
        const float b0 = rng.uni(-0.002f, 0.002f);
        const float y = rng.uni(-1.0f, 1.0f), z = rng.uni(-1.0f, 1.0f);
        V3 d = rng.dir();
        if (i & 1) {  // slopes around the threshold, unit length kept
            const float u = rng.uni(K - 0.12f, K + 0.12f), w = std::sqrt(1.0f - u * u), a = rng.uni(-3.1416f, 3.1416f);
            d = V3{u, w * std::cos(a), w * std::sin(a)};
        }
        const Ray s = on_face(Ray{V3{1.0f + b0, y, z}, d}, (int)(i % 6));
        const float maxt = rng.uni(40.0f, 60.0f);  // |lightPos - p| of the scene
        const bool acc = check_ray(s, maxt, (i & 3) == 0);
        n_face++;
        acc_face += acc ? 1 : 0;
        const bool hole = std::fabs(y) < 1.0f / 3.0f && std::fabs(z) < 1.0f / 3.0f;
        acc_hole += acc && hole ? 1 : 0;
        // brute force: the kernels' own march (fast form, uncapped, settle exit)
        if (d.x > 0.0f) {
            const bool one = bits(soft_shadow(s, MINT, maxt, false, INT_MAX, true).res) == bits(1.0f);
            one_face += one ? 1 : 0;
            acc_of_one += one && acc ? 1 : 0;
        }
    }
    CHECK(acc_face > n_face / 10 && acc_hole > 1000);
    // origins far outside and anywhere around the cube
    const long n2 = 300000;
    for (long i = 0; i < n2; i++) {
        const float r = (i & 1) ? 8.0f : 1.5f;
        const Ray s{V3{rng.uni(-r, r), rng.uni(-r, r), rng.uni(-r, r)}, rng.dir()};
        acc_far += check_ray(s, rng.uni(0.5f, 60.0f), (i & 3) == 0) ? 1 : 0;
    }
    CHECK(acc_far > n2 / 20);
    std::printf("random rays: %ld on faces, %ld accepted (%ld of them over a hole); %ld around the cube, %ld accepted\n",
                n_face, acc_face, acc_hole, n2, acc_far);
    std::printf("brute force: %ld outgoing face rays march to exactly 1; the predicate accepts %ld of them (%.1f %%)\n",
                one_face, acc_of_one, 100.0 * (double)acc_of_one / (double)(one_face ? one_face : 1));
}

static float up(float x, int n) {
    for (int i = 0; i < n; i++) x = std::nextafter(x, std::numeric_limits<float>::infinity());
    return x;
}
static float down(float x, int n) {
    for (int i = 0; i < n; i++) x = std::nextafter(x, -std::numeric_limits<float>::infinity());
    return x;
}

static void directed_rays() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float den = 1.0e-40f, tiny = std::numeric_limits<float>::denorm_min();
    // 1. the slope threshold to adjacent floats, on every face; the other axes cannot pass (|o| = 0.3, 0.2)
    for (int f = 0; f < 6; f++)
        for (int k = -3; k <= 3; k++) {
            const float u = k < 0 ? down(K, -k) : up(K, k);
            const float w = std::sqrt(1.0f - u * u);
            for (float b0 : {0.0f, 0.001f, 0x1p-24f}) {
                const Ray s = on_face(Ray{V3{1.0f + b0, 0.3f, -0.2f}, V3{u, w, 0.0f}}, f);
                CHECK(check_ray(s, 54.0f) == (k >= 0));
            }
        }
    // 2. the offset threshold to adjacent floats: b0 + u mint against kRatio mint, for origins just inside the face
    for (float u : {K + 0.01f, 0.5f, 0.9f, 1.0f})
        for (int f = 0; f < 6; f++) {
            const float w = std::sqrt(std::fmax(0.0f, 1.0f - u * u));
            const float a0 = 1.0f - (u - K) * MINT;  // about the threshold
            long acc = 0, rej = 0;
            for (int k = -40; k <= 40; k++) {
                const float a = k < 0 ? down(a0, -k) : up(a0, k);
                const Ray s = on_face(Ray{V3{a, -0.25f, 0.4f}, V3{u, 0.0f, w}}, f);
                const bool want = fmaf(u, MINT, a - 1.0f) >= K * MINT;  // the header's own form
                CHECK(check_ray(s, 54.0f) == want);
                (want ? acc : rej)++;
            }
            CHECK(acc > 0 && rej > 0);  // the sweep straddles the threshold
        }
    // 3. b0 across [-0.002, 0.002] at slopes below, at and above the threshold
    for (int i = 0; i <= 400; i++) {
        const float b0 = -0.002f + 0.00001f * (float)i;
        for (float u : {K - 0.05f, K, K + 0.02f, 0.6f, 0.95f}) {
            const float w = std::sqrt(1.0f - u * u);
            const Ray s = on_face(Ray{V3{1.0f + b0, 0.7f, 0.1f}, V3{u, 0.6f * w, 0.8f * w}}, i % 6);
            const bool acc = check_ray(s, 54.0f, (i & 7) == 0);
            if (u < K) CHECK(!acc);
            if (u >= K && b0 >= 0.0f) CHECK(acc);
        }
    }
    // 4. edges and corners: two or three axes near 1, leaving through one, two or all of them
    for (float e1 : {-0.002f, 0.0f, 0.0015f})
        for (float e2 : {-0.002f, 0.0f, 0.0015f})
            for (float sx : {1.0f, -1.0f})
                for (float sy : {1.0f, -1.0f}) {
                    const float dz[3] = {0.0f, 0.3f, -0.6f};
                    for (float z : dz) {
                        const float l = 1.0f / std::sqrt(2.0f + z * z);
                        // across the edge outward on both axes / on one only / sliding along it
                        check_ray(Ray{V3{sx * (1.0f + e1), sy * (1.0f + e2), 0.5f}, V3{sx * l, sy * l, z * l}}, 54.0f);
                        check_ray(Ray{V3{sx * (1.0f + e1), sy * (1.0f + e2), 0.5f}, V3{sx * l, -sy * l, z * l}}, 54.0f);
                        check_ray(Ray{V3{sx * (1.0f + e1), sy * (1.0f + e2), 1.0f + e1}, V3{sx * 0.36f, sy * 0.36f, 0.86f}}, 54.0f);
                        check_ray(Ray{V3{sx * (1.0f + e1), sy * (1.0f + e2), -1.0f - e2}, V3{sx * 0.577f, sy * 0.577f, -0.577f}}, 54.0f);
                    }
                    // along the edge: no outward slope on either axis
                    CHECK(!check_ray(Ray{V3{sx * (1.0f + e1), sy * (1.0f + e2), 0.0f}, V3{0.0f, 0.0f, 1.0f}}, 54.0f));
                }
    // 5. maxt below mint (no step), equal to it, and just above it (one step)
    for (float maxt : {0.0f, -1.0f, 0.005f, MINT, up(MINT, 1), up(MINT, 2), 0.0101f, nan}) {
        const Ray s{V3{1.0005f, 0.2f, 0.9f}, V3{0.6f, 0.0f, 0.8f}};
        CHECK(check_ray(s, maxt));
        CHECK(bits(soft_shadow(s, MINT, maxt, false, INT_MAX, true).res) == bits(1.0f));
    }
    // 6. zero and denormal direction components, both signs (the passing axis keeps its slope)
    for (float z : {0.0f, -0.0f, den, -den, tiny, -tiny})
        for (int f = 0; f < 6; f++) {
            CHECK(check_ray(on_face(Ray{V3{1.0f, 0.5f, 0.5f}, V3{1.0f, z, -z}}, f), 54.0f));
            CHECK(check_ray(on_face(Ray{V3{1.001f, -0.9f, 0.0f}, V3{0.6f, 0.8f, z}}, f), 54.0f));
            CHECK(!check_ray(on_face(Ray{V3{1.0f, 0.5f, 0.5f}, V3{z, 1.0f, 0.0f}}, f), 54.0f));  // parallel to the face
            CHECK(!check_ray(on_face(Ray{V3{1.0f, 0.5f, 0.5f}, V3{z, z, z}}, f), 54.0f));
        }
    // 7. non-finite input: refused, whichever component (and a non-finite or out-of-range mint)
    for (float bad : {inf, -inf, nan})
        for (int k = 0; k < 6; k++) {
            float v[6] = {1.001f, 0.5f, -0.25f, 0.8f, 0.6f, 0.0f};  // (accepted when finite)
            CHECK(rmsc::shadow_clear(v[0], v[1], v[2], v[3], v[4], v[5], MINT));
            v[k] = bad;
            CHECK(!rmsc::shadow_clear(v[0], v[1], v[2], v[3], v[4], v[5], MINT));
            for (int j = 0; j < 6; j++) {  // and with a second one
                float w[6] = {1.001f, 0.5f, -0.25f, 0.8f, 0.6f, 0.0f};
                w[k] = bad;
                w[j] = j == k ? bad : -inf;
                CHECK(!rmsc::shadow_clear(w[0], w[1], w[2], w[3], w[4], w[5], MINT));
            }
        }
    for (float m : {nan, inf, -inf, 0.0f, -0.01f, 0.001f, 2.0f}) CHECK(!rmsc::shadow_clear(1.001f, 0.5f, -0.25f, 0.8f, 0.6f, 0.0f, m));
    // other values of mint in range: the claim holds for them too
    for (float m : {0.01f, 0.02f, 0.1f, 1.0f}) CHECK(check_ray(Ray{V3{1.001f, 0.5f, -0.25f}, V3{0.8f, 0.6f, 0.0f}}, 54.0f, true, m));
    // origins past the predicate's range and directions longer than a rotated unit vector: refused
    CHECK(!rmsc::shadow_clear(2000.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, MINT));
    CHECK(!rmsc::shadow_clear(3.0e38f, 3.0e38f, 3.0e38f, 1.0f, 0.0f, 0.0f, MINT));
    CHECK(!rmsc::shadow_clear(1.001f, 0.0f, 0.0f, 1.01f, 0.0f, 0.0f, MINT));
    CHECK(!rmsc::shadow_clear(1.001f, 0.0f, 0.0f, 0.8f, 1.0e30f, 0.0f, MINT));
    CHECK(rmsc::shadow_clear(1.001f, 0.0f, 0.0f, 1.0f + 0x1p-10f, 0.0f, 0.0f, MINT));
    // 8. origins inside the cube (every |o_i| <= 0.99): never accepted, whatever the direction
    Rng rng{7};
    for (int i = 0; i < 200000; i++) {
        V3 o{rng.uni(-0.99f, 0.99f), rng.uni(-0.99f, 0.99f), rng.uni(-0.99f, 0.99f)};
        if (i % 4 == 1) o.x = (i & 4) ? 0.99f : -0.99f;
        if (i % 4 == 2) o.x = o.y = (i & 4) ? 0.99f : -0.99f;
        if (i % 4 == 3) o.x = o.y = o.z = 0.0f;
        CHECK(!clear(Ray{o, rng.dir()}));
    }
    // and a ray from outside aimed at the cube: its slope is inward
    for (int i = 0; i < 20000; i++) {
        const V3 d = rng.dir();
        const V3 target{rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f), rng.uni(-1.0f, 1.0f)};
        const float back = rng.uni(1.8f, 6.0f);  // (beyond sqrt(3): outside the cube on some axis)
        const Ray s{V3{target.x - d.x * back, target.y - d.y * back, target.z - d.z * back}, d};
        CHECK(!clear(s));
    }
}

int main() {
    CHECK(K >= 0.2f && K <= 0.5f);
    directed_rays();
    random_rays();
    std::printf("kRatio %.3f: accepted rays %ld, marches checked %ld, longest %ld steps, smallest h / mint on an accepted ray %.4f\n",
                (double)K, g_accepted, g_marches, g_longest, (double)g_min_ratio);
    std::printf("all checks passed\n");
    return 0;
}
