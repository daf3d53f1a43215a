// ccd_probe.cpp — continuous collision's arithmetic (include/spec/ccd.h) and the staging of its list (physics_amd/csrc/setup.hpp
// stage_ccd) with a host compiler alone: no HIP, no library (tests/test_ccd_cpu.py builds and runs it, once under the address and
// undefined-behaviour sanitizers; tests/test_gpu_ccd.py holds the kernel to it bit for bit). It runs every body against the ground
// and every static as the kernel (physics_amd/csrc/ccd.hip, k_ccd_sweep) runs them: the mover, the swept box against the static's
// fattened box (setup.hpp build_static_set makes it, as phys_set_static_bodies does), the filter, ccd_static_test, the least
// (t, id). Then it advances the body by dt * frac: the position half of the step (physics_amd/csrc/integrate.hip,
// integrate_position) restated here, since that is device code.
//
//   ccd_probe --staging <n_owned> [id ...]   prints the code of stage_ccd and the ids it kept (decimal)
//   ccd_probe <scene file>                   prints, per body, the bits of: frac target normal[3] pos[3] rot[4]
//
// Scene file, every number a 32-bit word in hex (floats by their bits):
//   n_statics n_bodies has_ground ground_y dt margin exact_rot filtered ground_filter
//   per static: shape pos[3] rot[4] half_extent[3] filter[2]
//   per body:   shape pos[3] rot[4] half_extent[3] lin[3] ang[3] filter[2]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spec/ccd.h"
#include "../../physics_amd/csrc/setup.hpp"

static uint32_t word(FILE* f) {
    unsigned v = 0;
    if (std::fscanf(f, "%x", &v) != 1) { std::fprintf(stderr, "scene file: short or malformed\n"); std::exit(2); }
    return (uint32_t)v;
}
static float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float real(FILE* f) { return u2f(word(f)); }
static v3 real3(FILE* f) { v3 r; r.x = real(f); r.y = real(f); r.z = real(f); return r; }
static quat real4(FILE* f) { quat q; q.i = real(f); q.j = real(f); q.k = real(f); q.w = real(f); return q; }

// RigidBody::step's position half (reference rigid_body.rs:28, 32-37) as integrate.hip states it
static void advance(int exact_rot, float dt, v3 v, v3 w, v3* x, quat* q) {
    x->x = x->x + v.x * dt;
    x->y = x->y + v.y * dt;
    x->z = x->z + v.z * dt;
    if (w.x != 0.0f || w.y != 0.0f || w.z != 0.0f) {
        const float nrm = v3_norm(w);
        if (!(nrm > 0.0f)) return;
        const v3 a = v3_div(w, nrm);
        const float theta = nrm * dt;
        const float scale = exact_rot ? theta : det_sinf(theta * 0.5f);
        const v3 u = v3_make((a.x * scale) / 2.0f, (a.y * scale) / 2.0f, (a.z * scale) / 2.0f);
        const float nn = v3_dot(u, u);
        const float eps = 1.1920929e-7f;
        quat dq;
        if (nn <= eps * eps) {
            dq.i = 0.0f; dq.j = 0.0f; dq.k = 0.0f; dq.w = 1.0f;
        } else {
            const float n = det_sqrtf(nn);
            const float f = 1.0f * det_sinf(n) / n;
            dq.i = u.x * f; dq.j = u.y * f; dq.k = u.z * f;
            dq.w = 1.0f * det_cosf(n);
        }
        *q = quat_mul(dq, *q);
    }
}

static int staging(int argc, char** argv) {
    const uint64_t n_owned = std::strtoull(argv[2], nullptr, 10);
    std::vector<uint32_t> ids;
    for (int k = 3; k < argc; ++k) ids.push_back((uint32_t)std::strtoull(argv[k], nullptr, 10));
    const phys::CcdStaging s = phys::stage_ccd(ids.size(), ids.empty() ? nullptr : ids.data(), n_owned);
    std::printf("%d", (int)s.code);
    for (uint32_t id : s.ids) std::printf(" %u", id);
    std::printf("\n%s\n", s.message.c_str());
    // null ids with entries, and the count's limit, which needs no array of that length
    const phys::CcdStaging a = phys::stage_ccd(3, nullptr, n_owned), b = phys::stage_ccd(1ull << 31, ids.data(), n_owned);
    std::printf("%d %d\n", (int)a.code, (int)b.code);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "--staging") == 0) return staging(argc, argv);
    if (argc != 2) { std::fprintf(stderr, "usage: ccd_probe --staging <n_owned> [id ...] | <scene file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t ns = word(f), nb = word(f), has_ground = word(f);
    const float ground_y = real(f), dt = real(f), margin = real(f);
    const uint32_t exact_rot = word(f), filtered = word(f), ground_filter = word(f);
    if (ns > (1u << 20) || nb > (1u << 20)) { std::fprintf(stderr, "scene file: counts out of range\n"); return 2; }
    std::vector<float> spos(3 * ns), srot(4 * ns), she(3 * ns);
    std::vector<uint32_t> sshape(ns), sfilt(2 * ns);
    for (uint32_t k = 0; k < ns; ++k) {
        sshape[k] = word(f);
        for (int a = 0; a < 3; ++a) spos[3 * k + a] = real(f);
        for (int a = 0; a < 4; ++a) srot[4 * k + a] = real(f);
        for (int a = 0; a < 3; ++a) she[3 * k + a] = real(f);
        sfilt[2 * k] = word(f); sfilt[2 * k + 1] = word(f);
    }
    phys::StaticSet set;
    if (ns) set = phys::build_static_set(ns, spos.data(), srot.data(), sshape.data(), she.data(), margin, 0.5f);
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t shape = word(f);
        v3 x = real3(f);
        quat q = real4(f);
        const v3 he = real3(f), v = real3(f), w = real3(f);
        const uint32_t fx = word(f), fy = word(f);
        const ccd_mover mv = ccd_mover_make(shape, x, q, he, v, dt);
        ccd_result best = ccd_result_none();
        v3 lo, hi;
        ccd_swept_aabb(&mv, &lo, &hi);
        if (mv.swept && has_ground && (!filtered || ccd_filter_pass(fx, fy, ground_filter, 0u))) {
            float t = 0.0f;
            const int res = ccd_ground_test(&mv, ground_y, &t);
            ccd_take(&best, &mv, res, t, v3_make(0.0f, 1.0f, 0.0f), CCD_GROUND);
        }
        for (uint32_t k = 0; mv.swept && k < ns; ++k) {
            const float* b = &set.box[8 * k];
            if (ccd_aabb_apart(lo, hi, v3_make(b[0], b[1], b[2]), v3_make(b[4], b[5], b[6]))) continue;
            if (filtered && !ccd_filter_pass(fx, fy, sfilt[2 * k], sfilt[2 * k + 1])) continue;
            const float* r = &set.rc[12 * k];
            bx_target tg;
            tg.shape = f2u(r[3]);
            tg.c = v3_make(r[0], r[1], r[2]);
            tg.q.i = r[4]; tg.q.j = r[5]; tg.q.k = r[6]; tg.q.w = r[7];
            tg.h = v3_make(r[8], r[9], r[10]);
            float t = 0.0f;
            v3 n = v3_make(0.0f, 0.0f, 0.0f);
            const int res = ccd_static_test(&mv, &tg, &t, &n);
            ccd_take(&best, &mv, res, t, n, f2u(r[11]));
        }
        ccd_finish(&best, &mv);
        advance(exact_rot != 0, dt * best.frac, v, w, &x, &q);
        std::printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", f2u(best.frac), best.target, f2u(best.n.x), f2u(best.n.y),
                    f2u(best.n.z), f2u(x.x), f2u(x.y), f2u(x.z), f2u(q.i), f2u(q.j), f2u(q.k), f2u(q.w));
    }
    std::fclose(f);
    return 0;
}
