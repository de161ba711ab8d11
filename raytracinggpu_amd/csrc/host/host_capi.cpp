// host_capi.cpp -- C exports of include/raytracer_host.h over the C++ host API (raytracer.hpp).
#include "../../../include/raytracer_host.h"
#include "../../../include/raytracer.hpp"
#include "../rt_qrows.h"
#include "../rt_still.h"
#include "../rt_rowcut.h"
#include "../rt_deadlast.h"
#include "../rt_gamma.h"

using namespace raytracer;

struct rth_mesh {
    TriangleMesh mesh;
    std::vector<float> arr;
};

extern "C" {

rth_mesh *rth_mesh_new(void) { return new (std::nothrow) rth_mesh(); }
void rth_mesh_free(rth_mesh *m) { delete m; }

int rth_mesh_read_obj(rth_mesh *m, const char *path, float scale, const float offset[3]) {
    FILE *f = std::fopen(path, "r");
    const bool ok = f != nullptr;
    if (f) std::fclose(f);
    m->mesh.obj_scale = scale;
    m->mesh.obj_offset = Vector(offset[0], offset[1], offset[2]);
    m->mesh.readOBJ(path);
    std::fflush(stdout);
    return ok ? 0 : -1;
}

void rth_mesh_set_arrays(rth_mesh *m, const float *v, int nv, const int32_t *t, int nt) {
    m->mesh.vertices.clear(); m->mesh.indices.clear();
    for (int i = 0; i < nv; ++i) m->mesh.vertices.push_back(Vector(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
    for (int i = 0; i < nt; ++i) m->mesh.indices.push_back(TriangleIndices(t[3 * i], t[3 * i + 1], t[3 * i + 2]));
    m->arr.clear();
}

void rth_mesh_rescale(rth_mesh *m, float scale, const float offset[3]) {
    m->mesh.rescale(scale, Vector(offset[0], offset[1], offset[2]));
}

int rth_mesh_build_bvh(rth_mesh *m) {
    m->arr = m->mesh.buildFlatBVH();
    return (int)m->mesh.n_bvhs;
}

int rth_mesh_num_vertices(const rth_mesh *m) { return (int)m->mesh.vertices.size(); }
int rth_mesh_num_triangles(const rth_mesh *m) { return (int)m->mesh.indices.size(); }
int rth_mesh_num_nodes(const rth_mesh *m) { return (int)(m->arr.size() / 10); }
void rth_mesh_get_vertices(const rth_mesh *m, float *o) {
    for (size_t i = 0; i < m->mesh.vertices.size(); ++i)
        for (int k = 0; k < 3; ++k) o[3 * i + k] = m->mesh.vertices[i][k];
}
void rth_mesh_get_indices(const rth_mesh *m, int32_t *o) {
    if (!m->mesh.indices.empty()) std::memcpy(o, &m->mesh.indices[0], m->mesh.indices.size() * sizeof(TriangleIndices));
}
void rth_mesh_get_bvh_array(const rth_mesh *m, float *o) {
    if (!m->arr.empty()) std::memcpy(o, m->arr.data(), m->arr.size() * sizeof(float));
}
int rth_write_png(const char *path, int W, int H, const uint8_t *rgb) { return write_png(path, W, H, rgb) ? 0 : -1; }

// the device's window arithmetic (rt_qrows.h) on the host, as wf_travq's fetch uses it: workgroup b of `tblocks` looks at window slots b * share + k, k < its share's length
int64_t rth_qrows_enumerate(int n_paths, int log2S, int Q, int tblocks, int which, int32_t info[4], int32_t *blk_len, int32_t *slots, int64_t cap) {
    using namespace rtk;
    const int S = 1 << log2S;
    const QRows w = which == 1 ? qrows_y(n_paths, log2S, Q) : which == 2 ? qrows_x(n_paths, log2S, Q) : QRows{0, 0, 0u};
    const int64_t total = w.rows != 0 ? qrows_slots(w, Q) : (int64_t)S * Q * 4;
    const int share = qrows_share(total, tblocks);
    info[0] = w.row0; info[1] = w.rows; info[2] = share; info[3] = (int32_t)total;
    int64_t n = 0;
    for (int b = 0; b < tblocks; ++b) {
        const int len = w.rows != 0 ? qrows_share_len(total, share, b) : share;        // no window: every workgroup scans a whole share, padding included
        if (blk_len) blk_len[b] = len;
        for (int k = 0; k < len; ++k, ++n) {
            const int64_t v = (int64_t)b * share + k;
            if (slots && n < cap) slots[n] = w.rows != 0 ? qrows_slot(w, log2S, (int)v) : (int32_t)v;
        }
    }
    return n;
}

// the still view's state machine and chain plan (rt_still.h) without a device.  The events stand for what the render path does per chunk and per chain: op 0 sizes the
// three buffers as size_wavefront does (the records only when StillView::may_store_records says so) and calls begin with 8-byte keys made of the ids
int64_t rth_still_replay(const int32_t *ev, int n_ev, uint64_t counts[12], int32_t *rows, int64_t cap) {
    using namespace rtk;
    StillView v;
    int64_t buf[3] = {0, 0, 0}, next_buf = 1, n = 0;                        // the allocations of the three levels as made-up addresses (0: none yet)
    auto at = [](int64_t id) { return reinterpret_cast<const void *>((intptr_t)id); };
    for (int e = 0; e < n_ev; ++e) {
        const int32_t *x = ev + 5 * e;
        if (x[0] == 0) {                                                    // a chunk of level x[1]: ray key x[2], Scene x[3], the rest of the shading key x[4]
            const int64_t ray = x[2], shade[2] = {x[3], x[4]};
            if (x[1] >= 1 && !buf[0]) buf[0] = next_buf++;
            if (x[1] >= 2 && !buf[1]) buf[1] = next_buf++;
            if (x[1] >= 3 && !buf[2] && v.may_store_records(&shade[0], sizeof(shade[0]))) buf[2] = next_buf++;
            v.begin(x[1], &ray, sizeof(ray), shade, sizeof(shade), at(buf[0]), at(buf[1]), at(buf[2]));
        } else if (x[0] == 1) {                                             // a chain of part x[1] with x[2] segments; x[3]: 1 a mesh, 2 row windows, 4 a Y window, 8 a plain chain that takes the closing kernel
            const StillChain c = v.chain(x[1], buf[2] != 0);
            const StillPlan p = still_plan(c, x[2], (x[3] & 1) != 0, (x[3] & 2) != 0, (x[3] & 4) != 0, (x[3] & 8) != 0);
            for (int it = p.first - 1; it < (p.n > p.first ? p.n : p.first); ++it, ++n) {
                if (!rows || n >= cap) continue;
                int32_t *r = rows + 12 * n;
                const bool open = it == p.first - 1;                        // the opening launch, then the positions
                const StillStep z{false, kWinNone, false, p.open_m0, 0, p.open};
                const StillStep &s = open ? z : p.step[it];
                const int32_t row[12] = {e, open ? -1 : it, s.trav, s.win, s.trav_m0, s.m0, s.x0, s.adv, open ? p.kill_x : 0, c.hit, c.shadow, c.records};
                memcpy(r, row, sizeof(row));
            }
        } else if (x[0] == 2) v.mesh_changed();
        else if (x[0] == 3) v.shading_changed();
        else if (x[0] == 4 && buf[x[1]]) buf[x[1]] = next_buf++;            // level x[1]'s buffer is a new allocation
    }
    const StillLevel *lv[3] = {&v.hit, &v.shadow, &v.records};
    for (int k = 0; k < 12; ++k) counts[k] = lv[k / 4]->counts[k % 4];
    return n;
}

// the form of the wf_advance launch that a chain of these facts enqueues for step `adv` (rt_still.h adv_form, as enqueue_chain and launch_render_counts ask for it);
// lights: 0 one point light, 1 several, 2 some with a radius; adv: StillAdv.  -1: not built
int64_t rth_advance_form(int counting, int tex, int anim, int list, int lens, int lights, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}
int64_t rth_advance_form_shutter(int counting, int tex, int anim, int list, int lens, int lights, int shutter, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights, shutter != 0}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}
int64_t rth_advance_form_sky(int counting, int tex, int anim, int list, int lens, int lights, int shutter, int sky, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights, shutter != 0, sky != 0}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}
int64_t rth_advance_form_sky_sample(int counting, int tex, int anim, int list, int lens, int lights, int shutter, int sky, int sample, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights, shutter != 0, sky != 0, sample != 0}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}
int64_t rth_advance_form_emit(int counting, int tex, int anim, int list, int lens, int lights, int shutter, int sky, int sample, int emit, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights, shutter != 0, sky != 0, sample != 0, emit != 0}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}
int64_t rth_advance_form_fresnel(int counting, int tex, int anim, int list, int lens, int lights, int shutter, int sky, int sample, int emit, int fresnel, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights, shutter != 0, sky != 0, sample != 0, emit != 0, fresnel != 0}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}
int64_t rth_advance_form_gloss(int counting, int tex, int anim, int list, int lens, int lights, int shutter, int sky, int sample, int emit, int fresnel, int gloss, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights, shutter != 0, sky != 0, sample != 0, emit != 0, fresnel != 0, gloss != 0}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}
int64_t rth_advance_form_tint(int counting, int tex, int anim, int list, int lens, int lights, int shutter, int sky, int sample, int emit, int fresnel, int gloss, int tint, int adv) {
    const unsigned form = rtk::adv_form(rtk::AdvFacts{counting != 0, tex != 0, anim != 0, list != 0, lens != 0, lights, shutter != 0, sky != 0, sample != 0, emit != 0, fresnel != 0, gloss != 0, tint != 0}, adv);
    return form == rtk::kFormNotBuilt ? -1 : (int64_t)form;
}

// the cut of a call's rows into sub-frames (rt_rowcut.h), as cut_wavefront and launch_path ask for it
void rth_row_cut(const int32_t *cases, int n, int32_t *out) {
    using namespace rtk;
    for (int i = 0; i < n; ++i) {
        const int32_t *x = cases + 7 * i;
        int32_t *o = out + 52 * i;
        const Rows rows{x[0], x[1], x[2], x[3]};
        const RowCut c = split_rows(rows, x[4], x[5] != 0);
        memset(o, 0, 52 * sizeof(int32_t));
        o[0] = c.parts; o[1] = c.R; o[2] = c.G; o[3] = c.T;
        for (int j = 0; j < c.parts && j < kRowCutMaxParts; ++j) {
            const RowPart p = c.part(rows, j, x[6] != 0);
            const int32_t row[6] = {p.row0, p.n_rows, p.tile_rows, p.tile_step, p.out_tile0, p.out_tile_step};
            memcpy(o + 4 + 6 * j, row, sizeof(row));
        }
    }
}

// ... and into chunks, as launch_render walks them
int rth_row_chunks(const int32_t *cases, int n, int32_t *out, int cap) {
    using namespace rtk;
    int most = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t *x = cases + 6 * i;
        int32_t *o = out + (size_t)(3 + 5 * cap) * i;
        const Rows rows{x[0], x[1], x[2], x[3]};
        memset(o, 0, (size_t)(3 + 5 * cap) * sizeof(int32_t));
        RowChunks ch{0, rows.n_rows, 1};
        const bool cut = rows_need_chunks(rows, x[4], x[5]);
        if (cut) ch = chunk_rows(rows, x[4], x[5]);
        o[0] = ch.unit; o[1] = ch.per; o[2] = ch.n;
        most = ch.n > most ? ch.n : most;
        for (int k = 0; k < ch.n && k < cap; ++k) {
            const Rows r = cut ? ch.chunk(rows, k) : rows;
            const int32_t row[5] = {cut ? ch.first(k) : 0, r.row0, r.n_rows, r.tile_rows, r.tile_step};
            memcpy(o + 3 + 5 * k, row, sizeof(row));
        }
    }
    return most;
}

// the dead-last permission (rt_deadlast.h), as enqueue_chain asks for it
int rth_dead_last_scene_size(void) { return (int)sizeof(rtk::DeadLastScene); }
void rth_dead_last_permit(const int32_t *facts, const void *scenes, int n, int32_t *out) {
    const rtk::DeadLastScene *s = static_cast<const rtk::DeadLastScene *>(scenes);
    for (int i = 0; i < n; ++i) {
        const int32_t *f = facts + 4 * i;
        out[i] = rtk::dead_last_permit(f[0] != 0, f[1] != 0, f[2] != 0, f[3], s[i]) ? 1 : 0;
    }
}

// the progressive path's byte (rt_gamma.h), as accumulate_kernel computes it
void rth_gamma_byte(const float *c, int n, uint8_t *out) {
    for (int i = 0; i < n; ++i) out[i] = (uint8_t)rtk::gamma_byte_f(c[i]);
}

}  // extern "C"
