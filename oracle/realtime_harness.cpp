/*
 * realtime_harness.cpp -- TEST INFRASTRUCTURE (fixture generator), NOT PRODUCT CODE.
 *
 * Runs the device code of the reference's realtime_render.cu as ordinary host functions, one "thread" at a time, and
 * dumps what it computes as raw little-endian arrays; oracle/realtime_fixture.py packs them into
 * tests/golden/ref_realtime.npz.  Built only where the reference exists (oracle/Makefile target
 * _ref/realtime_harness); the binary and the filtered text it is built from live under oracle/_ref/ alone.
 *
 * How the CUDA / GL program becomes a g++ program: oracle/Makefile cuts the translation unit before its GL / CUDA host
 * code (`void transformMesh(`) and drops the GL and stb includes -- by text, not by line number -- into
 * _ref/realtime_filtered.inc, and oracle/ref_stubs/ stands in for <cuda_runtime.h>, <curand_kernel.h> and
 * <cuda_gl_interop.h> (empty qualifiers, plain vector structs, threadIdx / blockIdx / blockDim / gridDim as globals,
 * CUDA's mixed min / max overloads, a curandState that replays a queue).  The reference's own cutil_math.h is found
 * with -I; it is compiled as nvcc sees it (__CUDACC__ defined around it alone), so its host-only fall-backs, which
 * would collide with <math.h>, stay out.
 *
 * What is called, each directly: Camera::rotate, KernelLaunch (its camera ray is caught by a Geometry subclass of this
 * file whose intersect records the ray and reports a miss; the same call yields the progressive quotient's 8-bit
 * output for a pre-loaded accumbuffer), TriangleMesh::get_smooth_normal, transform, MoveLightSource, MoveObject.
 *
 *   realtime_harness basis     IN(n,2: yaw pitch)                       OUT(n,9: bx by bz)
 *   realtime_harness rays      CASES(n,8: W H fov Cx Cy Cz yaw pitch) JITTER(m,2: r1 r2)  OUT_PREFIX
 *                                  .rays.f32: per case (m, H, W, 6: O u)     .tan.f32: (n,2: tan(pov / 2), z)
 *   realtime_harness prog      ACCUM(n,3) FRAMENUMBER                    OUT_PREFIX
 *                                  .bytes.u8 (n,4)  .accum.f32 (n,3)  .disp.f32 (n,3)
 *   realtime_harness transform VERTS(nv,3) NORMALS(nn,3) CASES(k,12: R t) OUT_PREFIX   .v.f32 (k,nv,3)  .n.f32 (k,nn,3)
 *   realtime_harness smooth    VERTS NORMALS TRIS(nt,6 int32: v v v n n n) RAYS(nr,6: O u)  OUT(nr,nt,3)
 *   realtime_harness light     IN(n,5: L speed dt) STEPS                 OUT   STEPS == 0: (n,3), one step each;
 *                                                                              STEPS > 0: (STEPS,3), row 0 chained
 *   realtime_harness object    IN(n,7: C v dt)                           OUT(n,3)
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <vector>
#include <math.h>
#include <stdio.h>

#include "cuda_runtime.h"     /* oracle/ref_stubs */
#include "curand_kernel.h"
#define __CUDACC__ 1          /* for cutil_math.h alone: as nvcc compiles it */
#include "cutil_math.h"       /* the reference's own, -I$(REF) */
#undef __CUDACC__
#include "realtime_filtered.inc"   /* -I_ref: written by oracle/Makefile, never tracked */

template <typename T> static std::vector<T> load(const char *path, size_t cols) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END); long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
    if (cols && v.size() % cols) { fprintf(stderr, "%s: not a multiple of %zu values\n", path, cols); exit(2); }
    return v;
}
template <typename T> static void dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("fwrite"); exit(2); }
    fclose(f);
}
static void put(std::vector<float> &o, const Vector &v) { o.push_back(v[0]); o.push_back(v[1]); o.push_back(v[2]); }

/* the probe: the only object of the scene; records the ray it is asked about, then misses */
class Probe : public Geometry {
public:
    std::vector<float> *sink = nullptr;
    int calls = 0;
    bool intersect(const Ray &r, float &t, Vector &N) override {
        calls++;
        if (sink) { put(*sink, r.O); put(*sink, r.u); }
        return 0;
    }
};

/* one thread of KernelLaunch: pixel (x, y) of a W x H frame in a single block */
static void launch_pixel(Scene *s, float3 *output, float3 *accum, int framenumber, int W, int H, int x, int y, const float *r12) {
    blockIdx = uint3{0, 0, 0}; gridDim = dim3{1, 1, 1};
    blockDim = dim3{(unsigned)W, (unsigned)H, 1};
    threadIdx = uint3{(unsigned)x, (unsigned)y, 0};
    curand_replay(r12, 2);
    KernelLaunch(s, output, accum, framenumber, 0u, W, H, 1, 1);
}

static int cmd_basis(char **a) {
    auto in = load<float>(a[0], 2);
    std::vector<float> out;
    Camera *c = new Camera();
    for (size_t i = 0; i < in.size() / 2; i++) {
        c->yaw = in[2 * i]; c->pitch = in[2 * i + 1];
        c->rotate();
        put(out, c->bx); put(out, c->by); put(out, c->bz);
    }
    dump(a[1], out);
    return 0;
}

static int cmd_rays(char **a) {
    auto cases = load<float>(a[0], 8), jit = load<float>(a[1], 2);
    std::vector<float> rays, tans;
    Scene *s = new Scene();
    Probe *probe = new Probe();
    probe->sink = &rays;
    s->objects_size = 0;
    s->addObject(probe);
    for (size_t k = 0; k < cases.size() / 8; k++) {
        const float *c = &cases[8 * k];
        const int W = (int)c[0], H = (int)c[1];
        s->pov = c[2];
        s->cam.C = Vector(c[3], c[4], c[5]);
        s->cam.yaw = c[6]; s->cam.pitch = c[7];
        s->cam.rotate();
        /* this program's own evaluation of the expression KernelLaunch uses for z, on the float the kernel reads */
        volatile float pov = s->pov;
        float t = tan(pov / 2);
        tans.push_back(t); tans.push_back(-W / (2 * t));
        std::vector<float3> output((size_t)W * H), accum((size_t)W * H);
        for (size_t j = 0; j < jit.size() / 2; j++)
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const int before = probe->calls;
                    launch_pixel(s, output.data(), accum.data(), 1, W, H, x, y, &jit[2 * j]);
                    if (probe->calls != before + 1 || curand_replay_drawn != 2) { fprintf(stderr, "rays: %d probe calls, %d draws\n", probe->calls - before, curand_replay_drawn); return 3; }
                }
    }
    dump(std::string(a[2]) + ".rays.f32", rays);
    dump(std::string(a[2]) + ".tan.f32", tans);
    return 0;
}

static int cmd_prog(char **a) {
    auto acc = load<float>(a[0], 3);
    const int framenumber = atoi(a[1]);
    const int n = (int)(acc.size() / 3);
    Scene *s = new Scene();
    Probe *probe = new Probe();
    s->objects_size = 0;
    s->addObject(probe);
    s->pov = 1.5707964f;
    std::vector<float3> output(n), accum(n);
    for (int i = 0; i < n; i++) accum[i] = make_float3(acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]);
    const float r12[2] = {1.f, 1.f};
    for (int i = 0; i < n; i++) launch_pixel(s, output.data(), accum.data(), framenumber, n, 1, i, 0, r12);
    std::vector<unsigned char> bytes; std::vector<float> accum_out, disp;
    for (int i = 0; i < n; i++) {
        Colour c; c.c = output[i].z;
        bytes.push_back(c.components.x); bytes.push_back(c.components.y); bytes.push_back(c.components.z); bytes.push_back(c.components.w);
        accum_out.push_back(accum[i].x); accum_out.push_back(accum[i].y); accum_out.push_back(accum[i].z);
        const float3 d = accum[i] / framenumber;      /* cutil_math's operator/(float3, float), as the kernel calls it */
        disp.push_back(d.x); disp.push_back(d.y); disp.push_back(d.z);
    }
    dump(std::string(a[2]) + ".bytes.u8", bytes);
    dump(std::string(a[2]) + ".accum.f32", accum_out);
    dump(std::string(a[2]) + ".disp.f32", disp);
    return 0;
}

static std::vector<Vector> vectors(const std::vector<float> &f) {
    std::vector<Vector> v(f.size() / 3);
    for (size_t i = 0; i < v.size(); i++) v[i] = Vector(f[3 * i], f[3 * i + 1], f[3 * i + 2]);
    return v;
}

static int cmd_transform(char **a) {
    auto vf = load<float>(a[0], 3), nf = load<float>(a[1], 3), cases = load<float>(a[2], 12);
    std::vector<float> vo, no;
    for (size_t k = 0; k < cases.size() / 12; k++) {
        std::vector<Vector> v = vectors(vf), n = vectors(nf);
        const float *c = &cases[12 * k];
        const int threads = (int)std::max(v.size(), n.size()) + 3;       /* a few threads past both sizes, as a rounded-up grid has */
        blockIdx = uint3{0, 0, 0}; blockDim = dim3{(unsigned)threads, 1, 1}; gridDim = dim3{1, 1, 1};
        for (int i = 0; i < threads; i++) {
            threadIdx = uint3{(unsigned)i, 0, 0};
            transform(v.data(), (int)v.size(), n.data(), (int)n.size(), Vector(c[9], c[10], c[11]), c);
        }
        for (auto &x : v) put(vo, x);
        for (auto &x : n) put(no, x);
    }
    dump(std::string(a[3]) + ".v.f32", vo);
    dump(std::string(a[3]) + ".n.f32", no);
    return 0;
}

static int cmd_smooth(char **a) {
    auto vf = load<float>(a[0], 3), nf = load<float>(a[1], 3), rays = load<float>(a[3], 6);
    auto tris = load<int>(a[2], 6);
    std::vector<Vector> v = vectors(vf), n = vectors(nf);
    TriangleMesh *m = new TriangleMesh();
    m->vertices = v.data(); m->vertices_size = (int)v.size();
    m->normals = n.data(); m->normals_size = (int)n.size();
    std::vector<float> out;
    for (size_t r = 0; r < rays.size() / 6; r++) {
        const float *p = &rays[6 * r];
        Ray ray(Vector(p[0], p[1], p[2]), Vector(p[3], p[4], p[5]));
        for (size_t t = 0; t < tris.size() / 6; t++) {
            const int *q = &tris[6 * t];
            Vector N;
            m->get_smooth_normal(ray, TriangleIndices(q[0], q[1], q[2], q[3], q[4], q[5]), N);
            put(out, N);
        }
    }
    dump(a[4], out);
    return 0;
}

static int cmd_light(char **a) {
    auto in = load<float>(a[0], 5);
    const int steps = atoi(a[1]);
    Scene *s = new Scene();
    std::vector<float> out;
    blockIdx = uint3{0, 0, 0}; threadIdx = uint3{0, 0, 0}; blockDim = dim3{1, 1, 1}; gridDim = dim3{1, 1, 1};
    const size_t rows = steps > 0 ? 1 : in.size() / 5;
    for (size_t i = 0; i < rows; i++) {
        const float *p = &in[5 * i];
        s->L = Vector(p[0], p[1], p[2]);
        for (int k = 0; k < (steps > 0 ? steps : 1); k++) {
            MoveLightSource(s, p[3], p[4]);
            put(out, s->L);
        }
    }
    dump(a[2], out);
    return 0;
}

static int cmd_object(char **a) {
    auto in = load<float>(a[0], 7);
    Scene *s = new Scene();
    Sphere *sp = new Sphere();
    s->objects_size = 0;
    s->objects[s->objects_size++] = sp;
    std::vector<float> out;
    blockIdx = uint3{0, 0, 0}; threadIdx = uint3{0, 0, 0}; blockDim = dim3{1, 1, 1}; gridDim = dim3{1, 1, 1};
    for (size_t i = 0; i < in.size() / 7; i++) {
        const float *p = &in[7 * i];
        sp->C = Vector(p[0], p[1], p[2]);
        MoveObject(s, 0, Vector(p[3], p[4], p[5]), p[6]);
        put(out, sp->C);
    }
    dump(a[1], out);
    return 0;
}

int main(int argc, char **argv) {
    struct { const char *name; int nargs; int (*fn)(char **); } cmds[] = {
        {"basis", 2, cmd_basis}, {"rays", 3, cmd_rays}, {"prog", 3, cmd_prog}, {"transform", 4, cmd_transform},
        {"smooth", 5, cmd_smooth}, {"light", 3, cmd_light}, {"object", 2, cmd_object}};
    for (auto &c : cmds)
        if (argc >= 2 && !strcmp(argv[1], c.name) && argc == 2 + c.nargs) return c.fn(argv + 2);
    fprintf(stderr, "usage: realtime_harness basis|rays|prog|transform|smooth|light|object FILES... (see the head of realtime_harness.cpp)\n");
    return 1;
}
