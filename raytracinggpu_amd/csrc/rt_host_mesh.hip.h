// rt_host_mesh.hip.h -- host side, part 4 of 4 (inside rt_capi.hip's extern "C" block): the entry points that change the uploaded meshes on the device -- smooth normals,
// transform + refit, rebuild of the reference's tree, the LBVH builder and its device-side install.  ctx->parts is the one record of the meshes and a one-mesh scene is a forest
// of one: every operation has ONE body, written over MeshPart ranges, and the public entries (plain: the scene's one mesh, for transform every mesh; rt_mesh_*_of: the mesh at an
// object slot) check their own preconditions and call it.  Only the device-side LBVH install is special to a scene of one mesh.
#pragma once

// Every node box recomputed for the tree in use (refit_kernel: the forest's synthetic nodes widened as build_forest makes them), the root box and the box filter's
// scene-wide quantities fetched, the fixed-point nodes derived again.  A whole-forest pass: the quantisation grid hangs on the root box.
// wide (rt_mesh_set_vertices* only): the boxes by the climb across the chip (rt_meshops.hip.h refit_up_kernel), bit for bit what refit_kernel makes of the same tree.
// Either way the entry then waits on its stream for the root box (32 bytes): the box travels to the render kernels as an argument and the quantisation grid hangs on it.
static int refit_and_requantize(rt_ctx *ctx, const bool wide = false) {
    ctx->still.mesh_changed();
    rtk::Scene &sc = ctx->scene;
    rtk::RefitArgs a{};
    a.node_lo = static_cast<float4 *>(ctx->node_lo.p); a.node_hi = static_cast<float4 *>(ctx->node_hi.p);
    a.nodes2 = static_cast<float4 *>(ctx->nodes2.p); a.nodesq = static_cast<float4 *>(ctx->nodesq.p); a.nodesb = static_cast<float4 *>(ctx->nodesb.p);
    a.q2thr = static_cast<const int *>(ctx->q2thr.p); a.left_of = static_cast<const int *>(ctx->left_dev.p);
    a.lvl_nodes = static_cast<const int *>(ctx->lvl_nodes.p); a.lvl_off = static_cast<const int *>(ctx->lvl_off.p);
    a.tidx = static_cast<const int4 *>(ctx->tidx.p); a.verts = static_cast<const float4 *>(ctx->verts.p);
    a.n_nodes = sc.n_nodes; a.n_levels = ctx->n_levels;
    a.n_syn = ctx->n_syn;
    for (int k = 0; k < ctx->n_syn; ++k) a.syn[k] = ctx->syn[k];
    if (!wide) {
        hipLaunchKernelGGL(rtk::refit_kernel, dim3(1), dim3(1024), 0, own_stream(ctx), a);
    } else {
        const size_t bytes = (size_t)sc.n_nodes * sizeof(int);
        if (int rc = ensure(ctx, ctx->refit_parent, bytes); rc != RT_OK) return rc;
        if (int rc = ensure(ctx, ctx->refit_cnt, bytes); rc != RT_OK) return rc;
        rtk::RefitWide w{a, static_cast<int *>(ctx->refit_parent.p), static_cast<int *>(ctx->refit_cnt.p)};
        hipStream_t q = own_stream(ctx);
        RT_HIP(ctx, hipMemsetAsync(w.parent, 0xff, bytes, q));                      // -1: the root's parent, and that of a node no internal node names
        RT_HIP(ctx, hipMemsetAsync(w.cnt, 0, bytes, q));
        const dim3 gn((unsigned)((sc.n_nodes + 255) / 256)), gc((unsigned)((sc.n_nodes + 1 + 255) / 256)), blk(256);
        hipLaunchKernelGGL(rtk::refit_parent_kernel, gn, blk, 0, q, w);
        hipLaunchKernelGGL(rtk::refit_up_kernel, gn, blk, 0, q, w);
        hipLaunchKernelGGL(rtk::refit_copy_kernel, gc, blk, 0, q, a);
    }
    RT_HIP(ctx, hipGetLastError());
    // the root box travels as a kernel argument (uniform root-box pre-test): fetch the refitted one
    float4 root[2];
    RT_HIP(ctx, hipMemcpyAsync(&root[0], ctx->node_lo.p, sizeof(float4), hipMemcpyDeviceToHost, own_stream(ctx)));
    RT_HIP(ctx, hipMemcpyAsync(&root[1], ctx->node_hi.p, sizeof(float4), hipMemcpyDeviceToHost, own_stream(ctx)));
    RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx)));
    sc.root_lo = root[0]; sc.root_hi = root[1];
    // the refitted root box contains every node's (unions, bottom-up): it bounds the magnitudes wf_travq's box filter needs
    const float rv[6] = {root[0].x, root[0].y, root[0].z, root[1].x, root[1].y, root[1].z};
    bool fast = true;
    float bm[3];
    for (int k = 0; k < 3; ++k) {
        if (!(rv[k] <= rv[k + 3]) || !(std::fabs(rv[k]) < 1e8f) || !(std::fabs(rv[k + 3]) < 1e8f)) fast = false;
        bm[k] = std::max(std::fabs(rv[k]), std::fabs(rv[k + 3]));
    }
    sc.bmx = bm[0]; sc.bmy = bm[1]; sc.bmz = bm[2];
    sc.fast_box = fast ? 1 : 0;
    return requantize(ctx, own_stream(ctx));                                          // the fixed-point pairs follow the refitted boxes (same topology: q16_topo_ok stands; unions nest)
}

// The per-mesh entries' common prologue: the record of the mesh at object_slot -- nullptr for a mesh without triangles, which the entries accept as a no-op.
static int find_part(rt_ctx *ctx, int object_slot, rt_ctx::MeshPart *&part) {
    part = nullptr;
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    const rtk::Scene &sc = ctx->scene;
    if (object_slot < 0 || object_slot >= sc.n_objects) return fail(ctx, RT_ERR_INVALID, "object_slot %d outside [0,%d)", object_slot, sc.n_objects);
    bool mesh = false;
    for (int k = 0; k < sc.n_meshes; ++k) mesh = mesh || sc.mesh[k].obj == object_slot;
    if (!mesh) return fail(ctx, RT_ERR_INVALID, "object_slot %d holds a sphere, not a TriangleMesh", object_slot);
    for (rt_ctx::MeshPart &p : ctx->parts) if (p.obj == object_slot) part = &p;
    return RT_OK;
}

// [vb, ve): the triangles (visit order) of the mesh at object position obj -- the forest stores them mesh after mesh (rtk::MeshRec)
static void visit_range(const rtk::Scene &sc, int obj, int &vb, int &ve) {
    vb = ve = 0;
    for (int k = 0; k < sc.n_meshes; ++k)
        if (sc.mesh[k].obj == obj) { vb = sc.mesh[k].tri_begin; ve = k + 1 < sc.n_meshes ? sc.mesh[k + 1].tri_begin : sc.n_tris; }
}

// One part's per-corner attribute (normals, UVs) in visit order: out[3 * (t - vb) + k] = the caller's index for corner k of the triangle at visit rank t of the part's range
// [vb, ...); the caller's rows are in the part's own uploaded triangle order.  `what` names the attribute in the message; indices lie in [0, n_vals).
static int gather_corners(rt_ctx *ctx, const rt_ctx::MeshPart &p, const char *what, const int32_t *idx, int index_stride, int n_triangles, int n_vals, int &vb, std::vector<int> &out) {
    if (int rr = refresh_host_mesh(ctx); rr != RT_OK) return rr;
    int ve;
    visit_range(ctx->scene, p.obj, vb, ve);
    out.resize(3 * (size_t)(ve - vb));
    for (int t = vb; t < ve; ++t) {
        const int src = ctx->tri_perm[t] - p.tri_off;                               // the mesh's own triangle index, uploaded order
        if (src < 0 || src >= p.nt) return fail(ctx, RT_ERR_INTERNAL, "visit rank %d is not a triangle of object %d", t, p.obj);
        if (src >= n_triangles) return fail(ctx, RT_ERR_INVALID, "n_triangles %d does not cover the mesh at object_slot %d (%d triangles)", n_triangles, p.obj, p.nt);
        for (int k = 0; k < 3; ++k) {
            const int i = idx[(size_t)src * index_stride + k];
            if (i < 0 || i >= n_vals) return fail(ctx, RT_ERR_INVALID, "triangle %d references %s %d outside [0,%d)", src, what, i, n_vals);
            out[3 * (size_t)(t - vb) + k] = i;
        }
    }
    return RT_OK;
}

// Smooth normals of one part: its range of `nrm` (one buffer for the scene, 3 normals per triangle in visit order; the entries of a flat mesh are never read) and its bit
static int set_part_normals(rt_ctx *ctx, rt_ctx::MeshPart &p, const float *normals_xyz, int n_normals, const int32_t *nidx, int index_stride, int n_triangles) {
    int vb;
    std::vector<int> ni;
    if (int rc = gather_corners(ctx, p, "normal", nidx, index_stride, n_triangles, n_normals, vb, ni); rc != RT_OK) return rc;
    std::vector<float4> nr(ni.size());
    for (size_t i = 0; i < ni.size(); ++i) nr[i] = make_float4(normals_xyz[3 * (size_t)ni[i]], normals_xyz[3 * (size_t)ni[i] + 1], normals_xyz[3 * (size_t)ni[i] + 2], 0.f);
    ctx->still.shading_changed();
    rtk::Scene &sc = ctx->scene;
    const size_t bytes = 3 * (size_t)sc.n_tris * sizeof(float4);
    if (sc.nrm == nullptr) {
        if (int rc = ensure(ctx, ctx->nrm, bytes); rc != RT_OK) return rc;
        RT_HIP(ctx, hipMemset(ctx->nrm.p, 0, bytes));
    }
    if (!nr.empty()) RT_HIP(ctx, hipMemcpy(static_cast<float4 *>(ctx->nrm.p) + 3 * (size_t)vb, nr.data(), nr.size() * sizeof(float4), hipMemcpyHostToDevice));
    p.smooth = true;
    sc.smooth_mask |= 1 << p.obj;
    sc.nrm = static_cast<const float4 *>(ctx->nrm.p);
    return RT_OK;
}

int rt_mesh_set_normals(rt_ctx *ctx, const float *normals_xyz, int n_normals, const int32_t *nidx, int index_stride, int n_triangles) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx)));
    if (!normals_xyz || !nidx) {                                                  // back to flat shading (every mesh)
        ctx->still.shading_changed();
        ctx->scene.nrm = nullptr; ctx->scene.smooth_mask = 0;
        for (rt_ctx::MeshPart &p : ctx->parts) p.smooth = false;
        return RT_OK;
    }
    if (ctx->parts.size() > 1) return fail(ctx, RT_ERR_UNSUPPORTED, "the scene holds %d meshes: smooth normals are set for ONE TriangleMesh", (int)ctx->parts.size());
    if (ctx->scene.mesh_slot < 0) return fail(ctx, RT_ERR_INVALID, "the scene has no mesh");
    if (n_normals <= 0 || index_stride < 3) return fail(ctx, RT_ERR_INVALID, "bad normal array sizes");
    if (ctx->parts.empty()) return RT_OK;                                         // a mesh without triangles: never hit, nothing to shade
    return set_part_normals(ctx, ctx->parts[0], normals_xyz, n_normals, nidx, index_stride, n_triangles);
}

int rt_mesh_set_normals_of(rt_ctx *ctx, int object_slot, const float *normals_xyz, int n_normals, const int32_t *nidx, int index_stride, int n_triangles) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    if (!p) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx)));
    if (!normals_xyz || !nidx) {                                                    // this mesh flat again
        ctx->still.shading_changed();
        rtk::Scene &sc = ctx->scene;
        p->smooth = false;
        sc.smooth_mask &= ~(1 << object_slot);
        if (sc.smooth_mask == 0) sc.nrm = nullptr;                                  // no smooth mesh left: the frames take the flat branch as before
        return RT_OK;
    }
    if (n_normals <= 0 || index_stride < 3) return fail(ctx, RT_ERR_INVALID, "bad normal array sizes");
    return set_part_normals(ctx, *p, normals_xyz, n_normals, nidx, index_stride, n_triangles);
}

// The reference's transformMesh (global_launcher.cu:932-946) on the parts [first, last): each part's vertices, its normals if it is smooth (rotated AND translated, as the
// reference's kernel does: global_launcher.cu:357-363; a flat part's slots of `nrm` are read by nothing and rewritten whole when it turns smooth), the triangle records of its
// visit range; then the whole-forest refit.
static int transform_parts(rt_ctx *ctx, size_t first, size_t last, const float rotation[9], const float translation[3]) {
    rtk::Scene &sc = ctx->scene;
    ctx->still.mesh_changed();
    if (sc.n_nodes <= 0 || sc.n_verts <= 0) return RT_OK;                           // no mesh, or no triangle in any leaf: nothing to move or refit
    RT_HIP(ctx, hipSetDevice(ctx->device));
    rtk::Mat3 m;
    for (int k = 0; k < 9; ++k) m.r[k] = rotation[k];
    for (int k = 0; k < 3; ++k) m.t[k] = translation[k];
    hipStream_t q = own_stream(ctx);
    for (size_t k = first; k < last; ++k) {
        const rt_ctx::MeshPart &p = ctx->parts[k];
        int vb, ve;
        visit_range(sc, p.obj, vb, ve);
        hipLaunchKernelGGL(rtk::transform_kernel, dim3((unsigned)((p.nv + 255) / 256)), dim3(256), 0, q, static_cast<float4 *>(ctx->verts.p) + p.voff, p.nv, m);
        if (ve <= vb) continue;
        if (p.smooth && sc.nrm != nullptr)
            hipLaunchKernelGGL(rtk::transform_kernel, dim3((unsigned)((3 * (ve - vb) + 255) / 256)), dim3(256), 0, q, static_cast<float4 *>(ctx->nrm.p) + 3 * (size_t)vb, 3 * (ve - vb), m);
        hipLaunchKernelGGL(rtk::retri_kernel, dim3((unsigned)((ve - vb + 255) / 256)), dim3(256), 0, q,
                           static_cast<const int4 *>(ctx->tidx.p) + vb, static_cast<const float4 *>(ctx->verts.p), static_cast<float4 *>(ctx->tri.p) + 3 * (size_t)vb, ve - vb);
    }
    RT_HIP(ctx, hipGetLastError());
    return refit_and_requantize(ctx);
}

int rt_mesh_transform(rt_ctx *ctx, const float rotation[9], const float translation[3]) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!rotation || !translation) return fail(ctx, RT_ERR_INVALID, "rotation/translation is NULL");
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    return transform_parts(ctx, 0, ctx->parts.size(), rotation, translation);      // every mesh
}

int rt_mesh_transform_of(rt_ctx *ctx, int object_slot, const float rotation[9], const float translation[3]) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!rotation || !translation) return fail(ctx, RT_ERR_INVALID, "rotation/translation is NULL");
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    if (!p) return RT_OK;                                                           // a mesh without triangles: nothing to move
    const size_t k = p - ctx->parts.data();
    return transform_parts(ctx, k, k + 1, rotation, translation);
}

// New positions for every vertex of one part (a mesh that changes shape: skinned, simulated, morphing), from the host (xyz_host: nv * 3 floats) or from device memory (xyz_dev:
// records `stride` floats apart, read on the context's stream); then what transform_parts does after its transform_kernel: the triangle records of the part's visit range and
// the whole-forest refit.  Indices, topology, visit order, materials, normals, UVs and textures stay.  The arguments were checked by the entries.
static int set_part_vertices(rt_ctx *ctx, const rt_ctx::MeshPart &p, const float *xyz_host, const void *xyz_dev, int stride) {
    rtk::Scene &sc = ctx->scene;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t q = own_stream(ctx);
    float4 *dst = static_cast<float4 *>(ctx->verts.p) + p.voff;
    if (xyz_host) {
        std::vector<float4> hv((size_t)p.nv);
        for (int i = 0; i < p.nv; ++i) hv[i] = make_float4(xyz_host[3 * (size_t)i], xyz_host[3 * (size_t)i + 1], xyz_host[3 * (size_t)i + 2], 0.f);
        RT_HIP(ctx, hipMemcpyAsync(dst, hv.data(), hv.size() * sizeof(float4), hipMemcpyHostToDevice, q));
        RT_HIP(ctx, hipStreamSynchronize(q));                                       // (the source lives on this stack frame)
    } else {
        hipLaunchKernelGGL(rtk::repack_vertices_kernel, dim3((unsigned)((p.nv + 255) / 256)), dim3(256), 0, q, static_cast<const float *>(xyz_dev), stride, dst, p.nv);
    }
    int vb, ve;
    visit_range(sc, p.obj, vb, ve);
    if (ve > vb)
        hipLaunchKernelGGL(rtk::retri_kernel, dim3((unsigned)((ve - vb + 255) / 256)), dim3(256), 0, q,
                           static_cast<const int4 *>(ctx->tidx.p) + vb, static_cast<const float4 *>(ctx->verts.p), static_cast<float4 *>(ctx->tri.p) + 3 * (size_t)vb, ve - vb);
    RT_HIP(ctx, hipGetLastError());
    return refit_and_requantize(ctx, ctx->knobs.refit_wide != 0);
}

static int set_vertices_checked(rt_ctx *ctx, const rt_ctx::MeshPart *p, const float *xyz_host, const void *xyz_dev, int stride, int n_vertices) {
    if (!p) return RT_OK;                                                           // a mesh without triangles: never hit, no box depends on it
    if (n_vertices != p->nv) return fail(ctx, RT_ERR_INVALID, "n_vertices %d differs from the %d vertices the mesh at object_slot %d was uploaded with", n_vertices, p->nv, p->obj);
    return set_part_vertices(ctx, *p, xyz_host, xyz_dev, stride);
}

// the scene's one mesh, for the entries that take no slot: refused on a forest as rt_mesh_set_normals is
static int the_one_part(rt_ctx *ctx, rt_ctx::MeshPart *&part) {
    part = nullptr;
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (ctx->parts.size() > 1) return fail(ctx, RT_ERR_UNSUPPORTED, "the scene holds %d meshes: name ONE TriangleMesh by its object slot (rt_mesh_set_vertices_of)", (int)ctx->parts.size());
    if (ctx->scene.mesh_slot < 0) return fail(ctx, RT_ERR_INVALID, "the scene has no mesh");
    if (!ctx->parts.empty()) part = &ctx->parts[0];
    return RT_OK;
}

int rt_mesh_set_vertices(rt_ctx *ctx, const float *xyz_host, int n_vertices) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = the_one_part(ctx, p); rc != RT_OK) return rc;
    if (!xyz_host) return fail(ctx, RT_ERR_INVALID, "xyz_host is NULL");
    return set_vertices_checked(ctx, p, xyz_host, nullptr, 3, n_vertices);
}

int rt_mesh_set_vertices_of(rt_ctx *ctx, int object_slot, const float *xyz_host, int n_vertices) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    if (!xyz_host) return fail(ctx, RT_ERR_INVALID, "xyz_host is NULL");
    return set_vertices_checked(ctx, p, xyz_host, nullptr, 3, n_vertices);
}

int rt_mesh_set_vertices_device(rt_ctx *ctx, int object_slot, const void *xyz_dev, int stride_floats, int n_vertices) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = object_slot == -1 ? the_one_part(ctx, p) : find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    if (!xyz_dev) return fail(ctx, RT_ERR_INVALID, "xyz_dev is NULL");
    if (stride_floats != 3 && stride_floats != 4) return fail(ctx, RT_ERR_INVALID, "stride_floats %d: positions are xyz (3) or xyzw (4) records", stride_floats);
    return set_vertices_checked(ctx, p, nullptr, xyz_dev, stride_floats, n_vertices);
}

// The positions of a mesh as they are now, kept for rt_render_aov_motion* (the previous corners of a deforming mesh's triangles): the part's range of `verts` copied into the
// same range of verts_prev, device to device on the context's stream -- behind the edits issued so far, ahead of those to come; the host does not wait.  A snapshot is
// nothing a render reads: the still-view state is not told.  A rebuild keeps it (it permutes tidx, and re-uploads `verts` value for value in the same order).
int rt_mesh_snapshot_vertices(rt_ctx *ctx, int object_slot, int keep) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    if (keep != 0 && keep != 1) return fail(ctx, RT_ERR_INVALID, "keep %d is neither 0 nor 1", keep);
    rt_ctx::MeshPart *one = nullptr;
    if (object_slot != -1) {
        if (int rc = find_part(ctx, object_slot, one); rc != RT_OK) return rc;
        if (!one) return RT_OK;                                                     // a mesh without triangles: never hit, nothing to keep
    }
    uint32_t bits = 0;
    for (const rt_ctx::MeshPart &p : ctx->parts) if (!one || &p == one) bits |= 1u << p.obj;
    if (!keep) { ctx->snap_mask &= ~bits; return RT_OK; }
    if (!bits) return RT_OK;
    if (int rc = ensure(ctx, ctx->verts_prev, (size_t)ctx->scene.n_verts * sizeof(float4)); rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    for (const rt_ctx::MeshPart &p : ctx->parts)
        if ((!one || &p == one) && p.nv > 0)
            RT_HIP(ctx, hipMemcpyAsync(static_cast<float4 *>(ctx->verts_prev.p) + p.voff, static_cast<const float4 *>(ctx->verts.p) + p.voff, (size_t)p.nv * sizeof(float4),
                                       hipMemcpyDeviceToDevice, own_stream(ctx)));
    if (!ctx->snap_ev) RT_HIP(ctx, ctx->snap_ev.create(hipEventDisableTiming));
    RT_HIP(ctx, hipEventRecord(ctx->snap_ev, own_stream(ctx)));
    ctx->snap_mask |= bits;
    return RT_OK;
}

int rt_mesh_snapshot_mask(const rt_ctx *ctx, uint32_t *mask) {
    if (!ctx || !mask) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    *mask = ctx->snap_mask;
    return RT_OK;
}

// The adjacency rt_mesh_compute_normals* walks (rt_normals.hip.h), for every vertex of the scene at once: a counting sort of the corners by the vertex they name, the
// triangles taken in ascending uploaded order (up_indices: as uploaded, or as the last rebuild reported -- the order gather_corners calls `src`), corners 0, 1, 2; what is
// stored is the triangle's visit rank (the inverse of tri_perm), where retri_kernel keeps its face normal.  A triangle in no leaf has no rank, no record and no part in
// any sum.  Built and uploaded once; install_scene and install_lbvh_device drop it.
static int ensure_vertex_csr(rt_ctx *ctx) {
    if (ctx->vcsr_valid) return RT_OK;
    if (int rr = refresh_host_mesh(ctx); rr != RT_OK) return rr;
    const int nv = ctx->scene.n_verts;
    const size_t nt = ctx->tri_perm.size();
    if (nt != (size_t)ctx->scene.n_tris || ctx->up_indices.size() != 3 * (size_t)ctx->n_up_tris) return fail(ctx, RT_ERR_INTERNAL, "the host's triangle orders do not describe the scene in use");
    std::vector<int> visit_of((size_t)ctx->n_up_tris, -1), off((size_t)nv + 1, 0), rank(3 * nt);
    for (size_t t = 0; t < nt; ++t) {
        const int g = ctx->tri_perm[t];
        if (g < 0 || g >= ctx->n_up_tris) return fail(ctx, RT_ERR_INTERNAL, "visit rank %zu names triangle %d outside [0,%d)", t, g, ctx->n_up_tris);
        visit_of[g] = (int)t;
    }
    size_t n_corners = 0;
    for (int g = 0; g < ctx->n_up_tris; ++g) {
        if (visit_of[g] < 0) continue;
        for (int k = 0; k < 3; ++k) {
            const int v = ctx->up_indices[3 * (size_t)g + k];
            if (v < 0 || v >= nv) return fail(ctx, RT_ERR_INTERNAL, "triangle %d references vertex %d outside [0,%d)", g, v, nv);
            ++off[(size_t)v + 1];
            ++n_corners;
        }
    }
    if (n_corners > rank.size()) return fail(ctx, RT_ERR_INTERNAL, "two visit ranks name one triangle");   // (cannot happen: visit_of holds one rank per triangle)
    for (int v = 0; v < nv; ++v) off[(size_t)v + 1] += off[v];
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int g = 0; g < ctx->n_up_tris; ++g) {
        if (visit_of[g] < 0) continue;
        for (int k = 0; k < 3; ++k) rank[(size_t)cur[ctx->up_indices[3 * (size_t)g + k]]++] = visit_of[g];
    }
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx)));                            // (an earlier adjacency may still be read by a launch on the stream)
    if (int rc = upload(ctx, ctx->vcsr_off, off.data(), off.size() * sizeof(int)); rc != RT_OK) return rc;
    if (int rc = upload(ctx, ctx->vcsr_rank, rank.data(), rank.size() * sizeof(int)); rc != RT_OK) return rc;
    ctx->vcsr_valid = true;
    return RT_OK;
}

// The vertex normals of one part's current shape, and the part shading with them: two launches on the context's stream behind the retri_kernel of the edits issued so far.
// After the first call (the adjacency, the buffers) the host waits for nothing.
static int compute_part_normals(rt_ctx *ctx, rt_ctx::MeshPart &p) {
    if (int rc = ensure_vertex_csr(ctx); rc != RT_OK) return rc;
    rtk::Scene &sc = ctx->scene;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t q = own_stream(ctx);
    if (int rc = ensure(ctx, ctx->vnrm, (size_t)sc.n_verts * sizeof(float4)); rc != RT_OK) return rc;
    const size_t bytes = 3 * (size_t)sc.n_tris * sizeof(float4);
    if (sc.nrm == nullptr) {                                                        // no smooth mesh so far: the other meshes' entries read as zeros, as set_part_normals leaves them
        if (int rc = ensure(ctx, ctx->nrm, bytes); rc != RT_OK) return rc;
        RT_HIP(ctx, hipMemsetAsync(ctx->nrm.p, 0, bytes, q));
    }
    ctx->still.shading_changed();
    int vb, ve;
    visit_range(sc, p.obj, vb, ve);
    if (p.nv > 0)
        hipLaunchKernelGGL(rtk::vertex_normals_kernel, dim3((unsigned)((p.nv + 255) / 256)), dim3(256), 0, q, static_cast<const int *>(ctx->vcsr_off.p),
                           static_cast<const int *>(ctx->vcsr_rank.p), static_cast<const float4 *>(ctx->tri.p), sc.n_tris, static_cast<float4 *>(ctx->vnrm.p), p.voff, p.nv);
    if (ve > vb)
        hipLaunchKernelGGL(rtk::corner_normals_kernel, dim3((unsigned)((3 * (size_t)(ve - vb) + 255) / 256)), dim3(256), 0, q, static_cast<const int4 *>(ctx->tidx.p) + vb,
                           static_cast<const float4 *>(ctx->vnrm.p), sc.n_verts, static_cast<float4 *>(ctx->nrm.p) + 3 * (size_t)vb, 3 * (ve - vb));
    RT_HIP(ctx, hipGetLastError());
    p.smooth = true;
    sc.smooth_mask |= 1 << p.obj;
    sc.nrm = static_cast<const float4 *>(ctx->nrm.p);
    ctx->vnrm_mask |= 1u << p.obj;
    return RT_OK;
}

int rt_mesh_compute_normals(rt_ctx *ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = the_one_part(ctx, p); rc != RT_OK) return rc;
    if (!p) return RT_OK;                                                           // a mesh without triangles: never hit, nothing to shade
    return compute_part_normals(ctx, *p);
}

int rt_mesh_compute_normals_of(rt_ctx *ctx, int object_slot) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    if (!p) return RT_OK;
    return compute_part_normals(ctx, *p);
}

// The per-vertex normals as the last rt_mesh_compute_normals* of that mesh wrote them (a later rt_mesh_transform* moves the corners' copies in `nrm`, not these)
int rt_mesh_get_vertex_normals(rt_ctx *ctx, int object_slot, float *out_xyz, int n_vertices) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = object_slot == -1 ? the_one_part(ctx, p) : find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    if (!out_xyz) return fail(ctx, RT_ERR_INVALID, "out_xyz is NULL");
    if (!p || !((ctx->vnrm_mask >> p->obj) & 1u) || !ctx->vnrm.p) return fail(ctx, RT_ERR_INVALID, "no vertex normals were computed for this mesh since the upload (rt_mesh_compute_normals*)");
    if (n_vertices != p->nv) return fail(ctx, RT_ERR_INVALID, "n_vertices %d differs from the %d vertices the mesh at object_slot %d was uploaded with", n_vertices, p->nv, p->obj);
    std::vector<float4> hv((size_t)p->nv);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipMemcpyAsync(hv.data(), static_cast<const float4 *>(ctx->vnrm.p) + p->voff, hv.size() * sizeof(float4), hipMemcpyDeviceToHost, own_stream(ctx)));
    RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx)));
    for (int i = 0; i < p->nv; ++i) { out_xyz[3 * (size_t)i] = hv[i].x; out_xyz[3 * (size_t)i + 1] = hv[i].y; out_xyz[3 * (size_t)i + 2] = hv[i].z; }
    return RT_OK;
}

// The shading normals of a smooth mesh as they are now, kept for rt_render_aov_motion* (N' of a smooth deforming mesh): the part's visit range of `nrm` copied into the same
// range of nrm_prev, as rt_mesh_snapshot_vertices copies `verts`.  A flat mesh has no shading normals to keep: its bit stays clear.  Nothing a render reads.
int rt_mesh_snapshot_normals(rt_ctx *ctx, int object_slot, int keep) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    if (keep != 0 && keep != 1) return fail(ctx, RT_ERR_INVALID, "keep %d is neither 0 nor 1", keep);
    rt_ctx::MeshPart *one = nullptr;
    if (object_slot != -1) {
        if (int rc = find_part(ctx, object_slot, one); rc != RT_OK) return rc;
        if (!one) return RT_OK;                                                     // a mesh without triangles: never hit, nothing to keep
    }
    const rtk::Scene &sc = ctx->scene;
    uint32_t bits = 0;
    for (const rt_ctx::MeshPart &p : ctx->parts)
        if ((!one || &p == one) && (!keep || (p.smooth && sc.nrm != nullptr))) bits |= 1u << p.obj;
    if (!keep) { ctx->nsnap_mask &= ~bits; return RT_OK; }
    if (!bits) return RT_OK;
    if (int rc = ensure(ctx, ctx->nrm_prev, 3 * (size_t)sc.n_tris * sizeof(float4)); rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    for (const rt_ctx::MeshPart &p : ctx->parts) {
        if (!((bits >> p.obj) & 1u)) continue;
        int vb, ve;
        visit_range(sc, p.obj, vb, ve);
        if (ve > vb)
            RT_HIP(ctx, hipMemcpyAsync(static_cast<float4 *>(ctx->nrm_prev.p) + 3 * (size_t)vb, static_cast<const float4 *>(ctx->nrm.p) + 3 * (size_t)vb,
                                       3 * (size_t)(ve - vb) * sizeof(float4), hipMemcpyDeviceToDevice, own_stream(ctx)));
    }
    if (!ctx->nsnap_ev) RT_HIP(ctx, ctx->nsnap_ev.create(hipEventDisableTiming));
    RT_HIP(ctx, hipEventRecord(ctx->nsnap_ev, own_stream(ctx)));
    ctx->nsnap_mask |= bits;
    return RT_OK;
}

int rt_mesh_normal_snapshot_mask(const rt_ctx *ctx, uint32_t *mask) {
    if (!ctx || !mask) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    *mask = ctx->nsnap_mask;
    return RT_OK;
}

// TriangleMesh::buildBVH on the device, bit for bit (rt_bvhbuild.hip.h): leaves the flat tree in ctx->bb_arr and the triangle order in ctx->bb_idx
// (up_off: the mesh's first triangle in tidx_up -- a forest's member; its vertex indices are global, the outputs are local to the mesh)
static int rebuild_reference_tree(rt_ctx *ctx, const int nt, int &n_nodes_out, const int up_off = 0) {
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cap = 2 * (size_t)nt + 2;                                          // nodes: every split makes two
    int rc;
    if ((rc = ensure(ctx, ctx->bb_idx, nt * sizeof(int))) != RT_OK || (rc = ensure(ctx, ctx->bb_cnt, nt * sizeof(int))) != RT_OK ||
        (rc = ensure(ctx, ctx->bb_pa, nt * sizeof(int))) != RT_OK || (rc = ensure(ctx, ctx->bb_pb, nt * sizeof(int))) != RT_OK ||
        (rc = ensure(ctx, ctx->bb_tmp, nt * sizeof(int))) != RT_OK || (rc = ensure(ctx, ctx->bb_nodes_i, 4 * cap * sizeof(int))) != RT_OK ||
        (rc = ensure(ctx, ctx->bb_nodes_f, 2 * cap * sizeof(float4))) != RT_OK || (rc = ensure(ctx, ctx->bb_counter, 2 * sizeof(int))) != RT_OK ||
        (rc = ensure(ctx, ctx->bb_lvl, (cap + 1) * sizeof(int))) != RT_OK || (rc = ensure(ctx, ctx->bb_size, cap * sizeof(int))) != RT_OK ||
        (rc = ensure(ctx, ctx->bb_pre, cap * sizeof(int))) != RT_OK || (rc = ensure(ctx, ctx->bb_arr, cap * 10 * sizeof(float))) != RT_OK)
        return rc;
    rtk::BuildArgs a{};
    a.verts = static_cast<const float4 *>(ctx->verts.p); a.tidx_up = static_cast<const int4 *>(ctx->tidx_up.p) + up_off;
    a.idx = static_cast<int *>(ctx->bb_idx.p); a.cnt = static_cast<int *>(ctx->bb_cnt.p);
    a.ptr_a = static_cast<int *>(ctx->bb_pa.p); a.ptr_b = static_cast<int *>(ctx->bb_pb.p); a.tmp = static_cast<int *>(ctx->bb_tmp.p);
    int *ni = static_cast<int *>(ctx->bb_nodes_i.p);
    a.n_start = ni; a.n_end = ni + cap; a.n_left = ni + 2 * cap; a.n_right = ni + 3 * cap;
    a.n_mn = static_cast<float4 *>(ctx->bb_nodes_f.p); a.n_mx = a.n_mn + cap;
    a.counter = static_cast<int *>(ctx->bb_counter.p); a.n_tris = nt; a.cap = (int)cap;
    hipStream_t q = own_stream(ctx);
    // root = node 0 over all triangles (buildBVH(&bvh, 0, T), cpu:684); the permutation starts as the identity
    hipLaunchKernelGGL(rtk::iota_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, q, a.idx, nt);
    const int root_range[2] = {0, nt}, one[2] = {1, 0};              // counter[0] = nodes allocated, counter[1] = a split was refused for lack of capacity
    RT_HIP(ctx, hipMemcpyAsync(a.n_start, &root_range[0], sizeof(int), hipMemcpyHostToDevice, q));
    RT_HIP(ctx, hipMemcpyAsync(a.n_end, &root_range[1], sizeof(int), hipMemcpyHostToDevice, q));
    RT_HIP(ctx, hipMemcpyAsync(a.counter, one, 2 * sizeof(int), hipMemcpyHostToDevice, q));
    RT_HIP(ctx, hipStreamSynchronize(q));                                           // the three sources above live on this stack frame
    std::vector<int> lvl_first{0};
    int first = 0, count = 1;
    while (count > 0) {                                                             // one launch per level, one workgroup per node
        hipLaunchKernelGGL(rtk::bvh_level_kernel, dim3((unsigned)count), dim3(rtk::kBuildThreads), 0, q, a, first);
        RT_HIP(ctx, hipGetLastError());
        int tot[2] = {0, 0};
        RT_HIP(ctx, hipMemcpyAsync(tot, a.counter, 2 * sizeof(int), hipMemcpyDeviceToHost, q));
        RT_HIP(ctx, hipStreamSynchronize(q));
        const int total = tot[0];
        // the kernel refuses a split that would pass the arrays' capacity (it cannot for a tree over nt triangles); the scene in use is untouched so far
        if (tot[1] != 0 || (size_t)total > cap) return fail(ctx, RT_ERR_INTERNAL, "BVH build needed more than %zu nodes for %d triangles (scene unchanged)", cap, nt);
        first += count;
        lvl_first.push_back(first);
        count = total - first;
    }
    const int n_nodes = first, n_levels = (int)lvl_first.size() - 1;
    n_nodes_out = n_nodes;
    if (n_nodes >= (1 << 24)) return fail(ctx, RT_ERR_INVALID, "node indices are stored as floats: < 2^24 nodes");
    RT_HIP(ctx, hipMemcpyAsync(ctx->bb_lvl.p, lvl_first.data(), lvl_first.size() * sizeof(int), hipMemcpyHostToDevice, q));
    hipLaunchKernelGGL(rtk::bvh_flatten_kernel, dim3(1), dim3(1024), 0, q, a, static_cast<const int *>(ctx->bb_lvl.p), n_levels,
                       static_cast<int *>(ctx->bb_size.p), static_cast<int *>(ctx->bb_pre.p), static_cast<float *>(ctx->bb_arr.p));
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// The LBVH builder (rt_lbvh.hip.h): Morton sort + parallel hierarchy emission, leaves cut by the surface-area heuristic (at most kLbvhLeaf = 32 triangles); same outputs
static int rebuild_lbvh_tree(rt_ctx *ctx, const int nt, int &n_nodes_out, const int up_off = 0) {
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t q = own_stream(ctx);
    const size_t n = (size_t)nt, nc = 2 * n - 1;
    int rc;
    DevBuf &B = ctx->lb_pool;
    // one pool, carved: keys (2 x 8n), vals (2 x 4n), 6 int arrays of n, flags, boxes (4 x 16n), alive + index (2 x 4 (2n)), bounds / stats
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_keys = carve(8 * n), o_keys2 = carve(8 * n), o_vals = carve(4 * n), o_vals2 = carve(4 * n);
    const size_t o_left = carve(4 * n), o_right = carve(4 * n), o_parent = carve(4 * n), o_first = carve(4 * n), o_last = carve(4 * n), o_lparent = carve(4 * n), o_flag = carve(4 * n), o_cost = carve(4 * n), o_leafify = carve(4 * n);
    const size_t o_ilo = carve(16 * n), o_ihi = carve(16 * n), o_llo = carve(16 * n), o_lhi = carve(16 * n);
    const size_t o_alive = carve(4 * nc), o_index = carve(4 * nc), o_small = carve(64);
    size_t sort_tmp = 0, scan_tmp = 0;
    {
        unsigned long long *k0 = nullptr; int *v0 = nullptr;
        if (rocprim::radix_sort_pairs(nullptr, sort_tmp, k0, k0, v0, v0, n, 0, 63, q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::radix_sort_pairs (size query) failed");
        if (rocprim::exclusive_scan(nullptr, scan_tmp, v0, v0, 0, nc, rocprim::plus<int>(), q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::exclusive_scan (size query) failed");
    }
    const size_t o_tmp = carve(std::max(sort_tmp, scan_tmp) + 256);
    if ((rc = ensure(ctx, B, off)) != RT_OK) return rc;
    if ((rc = ensure(ctx, ctx->bb_idx, n * sizeof(int))) != RT_OK) return rc;
    uint8_t *base = static_cast<uint8_t *>(B.p);
    rtk::LbvhArgs a{};
    // the leaf cut's triangle cost: kLbvhCt (wf_travq's step times on 64-byte pairs) for small trees; 1.0 for trees that will use the 32-byte fixed-point pairs, where a box test is
    // cheaper still but a triangle's 48-byte gather is not (swept on 524 288 / 2 M triangles: Ct 1.0 / 1.6 / 2.5 / 4 / 8 = 2.77 / 2.84 / 2.99 / 3.04 / 3.06 and 8.21 / 8.40 / 8.72 / 8.73 / 8.80 ms per frame)
    a.ct = ctx->knobs.lbvh_ct > 0.f ? ctx->knobs.lbvh_ct : (nt >= kQ16AutoNodes ? 1.0f : rtk::kLbvhCt); a.cb = rtk::kLbvhCb;
    a.verts = static_cast<const float4 *>(ctx->verts.p); a.tidx_up = static_cast<const int4 *>(ctx->tidx_up.p) + up_off; a.n = nt;
    a.bounds = reinterpret_cast<unsigned int *>(base + o_small); a.stats = reinterpret_cast<int *>(base + o_small + 32);
    a.keys = reinterpret_cast<unsigned long long *>(base + o_keys); a.vals = reinterpret_cast<int *>(base + o_vals);
    a.left = reinterpret_cast<int *>(base + o_left); a.right = reinterpret_cast<int *>(base + o_right); a.parent = reinterpret_cast<int *>(base + o_parent);
    a.first = reinterpret_cast<int *>(base + o_first); a.last = reinterpret_cast<int *>(base + o_last); a.leaf_parent = reinterpret_cast<int *>(base + o_lparent);
    a.flag = reinterpret_cast<int *>(base + o_flag);
    a.cost = reinterpret_cast<float *>(base + o_cost); a.leafify = reinterpret_cast<int *>(base + o_leafify);
    a.ibox_lo = reinterpret_cast<float4 *>(base + o_ilo); a.ibox_hi = reinterpret_cast<float4 *>(base + o_ihi);
    a.lbox_lo = reinterpret_cast<float4 *>(base + o_llo); a.lbox_hi = reinterpret_cast<float4 *>(base + o_lhi);
    a.alive = reinterpret_cast<int *>(base + o_alive); a.index = reinterpret_cast<int *>(base + o_index);
    const unsigned int binit[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    int zero4[4] = {0, 0, 0, 0};
    RT_HIP(ctx, hipMemcpyAsync(a.bounds, binit, sizeof(binit), hipMemcpyHostToDevice, q));
    RT_HIP(ctx, hipMemcpyAsync(a.stats, zero4, sizeof(zero4), hipMemcpyHostToDevice, q));
    RT_HIP(ctx, hipStreamSynchronize(q));                                        // (the two sources live on this stack frame)
    const dim3 gt((unsigned)((n + 255) / 256)), gc((unsigned)((nc + 255) / 256)), blk(256);
    hipLaunchKernelGGL(rtk::lbvh_bounds_kernel, gt, blk, 0, q, a);
    hipLaunchKernelGGL(rtk::lbvh_morton_kernel, gt, blk, 0, q, a);
    {   // (code, triangle) pairs by code; the sorted arrays become a.keys / a.vals
        unsigned long long *k2 = reinterpret_cast<unsigned long long *>(base + o_keys2);
        int *v2 = reinterpret_cast<int *>(base + o_vals2);
        size_t tmp = sort_tmp;
        if (rocprim::radix_sort_pairs(base + o_tmp, tmp, a.keys, k2, a.vals, v2, n, 0, 63, q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::radix_sort_pairs failed");
        a.keys = k2; a.vals = v2;
    }
    hipLaunchKernelGGL(rtk::lbvh_hierarchy_kernel, gt, blk, 0, q, a);
    hipLaunchKernelGGL(rtk::lbvh_boxes_kernel, gt, blk, 0, q, a);          // boxes + the leaf-or-subtree decision, bottom-up
    hipLaunchKernelGGL(rtk::lbvh_alive_kernel, gc, blk, 0, q, a);
    {
        size_t tmp = scan_tmp;
        if (rocprim::exclusive_scan(base + o_tmp, tmp, a.alive, a.index, 0, nc, rocprim::plus<int>(), q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::exclusive_scan failed");
    }
    RT_HIP(ctx, hipGetLastError());
    int last2[2] = {0, 0};                                                       // n_alive = index[last] + alive[last]
    RT_HIP(ctx, hipMemcpyAsync(&last2[0], a.index + (nc - 1), sizeof(int), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipMemcpyAsync(&last2[1], a.alive + (nc - 1), sizeof(int), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipStreamSynchronize(q));
    const int n_nodes = last2[0] + last2[1];
    if (n_nodes < 1 || (size_t)n_nodes > nc) return fail(ctx, RT_ERR_INTERNAL, "LBVH build: %d nodes for %d triangles (scene unchanged)", n_nodes, nt);
    if (n_nodes >= (1 << 24)) return fail(ctx, RT_ERR_INVALID, "node indices are stored as floats: < 2^24 nodes");
    if ((rc = ensure(ctx, ctx->bb_arr, (size_t)n_nodes * 10 * sizeof(float))) != RT_OK) return rc;
    a.arr10 = static_cast<float *>(ctx->bb_arr.p);
    hipLaunchKernelGGL(rtk::lbvh_emit_kernel, gc, blk, 0, q, a);
    RT_HIP(ctx, hipGetLastError());
    RT_HIP(ctx, hipMemcpyAsync(ctx->bb_idx.p, a.vals, n * sizeof(int), hipMemcpyDeviceToDevice, q));   // the triangle order, where the shared tail expects it
    int st[4] = {0, 0, 0, 0};
    RT_HIP(ctx, hipMemcpyAsync(st, a.stats, sizeof(st), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipStreamSynchronize(q));
    ctx->build.n_leaves = st[0]; ctx->build.max_leaf_tris = st[1]; ctx->build.max_depth = st[2];
    ctx->lb_args = a;
    n_nodes_out = n_nodes;
    return RT_OK;
}

// The render kernels' formats from the LBVH builder's arrays, on the device (rt_lbvh.hip.h, second half): what install_scene does on the
// host for an uploaded tree.  A scene of ONE part only (the builder ran over the whole of tidx_up).  `old`: the scene in use (spheres, light, camera, albedo, mesh slot carry over).
static int install_lbvh_device(rt_ctx *ctx, const rtk::Scene &old, const int n_nodes) {
    ctx->still.mesh_changed();
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t q = own_stream(ctx);
    const rtk::LbvhArgs &a = ctx->lb_args;
    const size_t n = (size_t)a.n, N = (size_t)n_nodes, nc = 2 * n - 1;
    int rc;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_flag = carve(4 * (n + 1)), o_scan = carve(4 * (n + 1)), o_X = carve(4 * N), o_bfs = carve(4 * N), o_key = carve(8 * N), o_key2 = carve(8 * N),
                 o_val = carve(4 * N), o_val2 = carve(4 * N), o_hist = carve(4 * 80), o_upnew = carve(16 * n);
    size_t sort_tmp = 0, scan_tmp = 0;
    {
        unsigned long long *k0 = nullptr; int *v0 = nullptr;
        if (rocprim::radix_sort_pairs(nullptr, sort_tmp, k0, k0, v0, v0, N, 0, 64, q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::radix_sort_pairs (size query) failed");
        if (rocprim::exclusive_scan(nullptr, scan_tmp, v0, v0, 0, n + 1, rocprim::plus<int>(), q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::exclusive_scan (size query) failed");
    }
    const size_t o_tmp = carve(std::max(sort_tmp, scan_tmp) + 256);
    if ((rc = ensure(ctx, ctx->lb_pool2, off)) != RT_OK) return rc;
    // the scene in use stays untouched until every allocation has succeeded
    DevBuf *outs[] = {&ctx->node_lo, &ctx->node_hi, &ctx->nodes2, &ctx->nodesq, &ctx->nodesb, &ctx->q2thr, &ctx->left_dev, &ctx->lvl_nodes, &ctx->lvl_off, &ctx->tri, &ctx->tidx, &ctx->perm_dev};
    const size_t need[] = {N * 16, N * 16, 2 * N * 16, 2 * (N + 1) * 16, 2 * (N + 1) * 16, (N + 1) * 4, N * 4, N * 4, 80 * 4, 3 * n * 16, n * 16, n * 4};
    ctx->have_scene = false;                                                     // (a failure from here on leaves the context without a scene, as the host path does)
    for (size_t k = 0; k < sizeof(need) / sizeof(need[0]); ++k) if ((rc = ensure(ctx, *outs[k], need[k])) != RT_OK) return rc;
    uint8_t *base = static_cast<uint8_t *>(ctx->lb_pool2.p);
    int *flag = reinterpret_cast<int *>(base + o_flag);
    rtk::LbvhLayout y{};
    y.n_nodes = n_nodes;
    y.lscan = reinterpret_cast<int *>(base + o_scan); y.X = reinterpret_cast<int *>(base + o_X); y.bfs = reinterpret_cast<int *>(base + o_bfs);
    y.bkey = reinterpret_cast<unsigned long long *>(base + o_key); y.bval = reinterpret_cast<int *>(base + o_val);
    y.dhist = reinterpret_cast<int *>(base + o_hist);
    y.node_lo = static_cast<float4 *>(ctx->node_lo.p); y.node_hi = static_cast<float4 *>(ctx->node_hi.p); y.nodes2 = static_cast<float4 *>(ctx->nodes2.p);
    y.nodesq = static_cast<float4 *>(ctx->nodesq.p); y.nodesb = static_cast<float4 *>(ctx->nodesb.p); y.q2thr = static_cast<int *>(ctx->q2thr.p);
    y.left_of = static_cast<int *>(ctx->left_dev.p); y.lvl_nodes = static_cast<int *>(ctx->lvl_nodes.p);
    y.tidx_visit = static_cast<int4 *>(ctx->tidx.p); y.tidx_up_new = reinterpret_cast<int4 *>(base + o_upnew); y.perm = static_cast<int *>(ctx->perm_dev.p);
    RT_HIP(ctx, hipMemsetAsync(flag, 0, 4 * (n + 1), q));
    RT_HIP(ctx, hipMemsetAsync(y.dhist, 0, 4 * 80, q));
    RT_HIP(ctx, hipMemsetAsync(y.nodesq, 0, 32, q));                              // entry 0 of the breadth-first arrays is padding
    RT_HIP(ctx, hipMemsetAsync(y.nodesb, 0, 32, q));
    RT_HIP(ctx, hipMemsetAsync(y.q2thr, 0, 4, q));
    const dim3 gt((unsigned)((n + 255) / 256)), gc((unsigned)((nc + 255) / 256)), gn((unsigned)((N + 255) / 256)), blk(256);
    hipLaunchKernelGGL(rtk::lbvh_leafflag_kernel, gc, blk, 0, q, a, flag);
    { size_t tmp = scan_tmp; if (rocprim::exclusive_scan(base + o_tmp, tmp, flag, y.lscan, 0, n + 1, rocprim::plus<int>(), q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::exclusive_scan failed"); }
    hipLaunchKernelGGL(rtk::lbvh_walk_kernel, gc, blk, 0, q, a, y);
    unsigned long long *key2 = reinterpret_cast<unsigned long long *>(base + o_key2);
    int *val2 = reinterpret_cast<int *>(base + o_val2);
    { size_t tmp = sort_tmp; if (rocprim::radix_sort_pairs(base + o_tmp, tmp, y.bkey, key2, y.bval, val2, N, 0, 64, q) != hipSuccess) return fail(ctx, RT_ERR_HIP, "rocprim::radix_sort_pairs failed"); }
    hipLaunchKernelGGL(rtk::lbvh_rank_kernel, gn, blk, 0, q, y, val2);
    const int4 *up_old = static_cast<const int4 *>(ctx->tidx_up.p);
    hipLaunchKernelGGL(rtk::lbvh_layout_kernel, gc, blk, 0, q, a, y, up_old);
    hipLaunchKernelGGL(rtk::lbvh_reorder_kernel, gt, blk, 0, q, a, up_old, y.tidx_up_new);
    RT_HIP(ctx, hipGetLastError());
    RT_HIP(ctx, hipMemcpyAsync(ctx->tidx_up.p, y.tidx_up_new, n * sizeof(int4), hipMemcpyDeviceToDevice, q));   // the sorted order is the new uploaded order
    hipLaunchKernelGGL(rtk::retri_kernel, gt, blk, 0, q, static_cast<const int4 *>(ctx->tidx.p), static_cast<const float4 *>(ctx->verts.p), static_cast<float4 *>(ctx->tri.p), (int)n);
    RT_HIP(ctx, hipGetLastError());
    int hist[65];
    float4 root[2];
    RT_HIP(ctx, hipMemcpyAsync(hist, y.dhist, sizeof(hist), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipMemcpyAsync(&root[0], ctx->node_lo.p, sizeof(float4), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipMemcpyAsync(&root[1], ctx->node_hi.p, sizeof(float4), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipStreamSynchronize(q));
    const int maxd = hist[64];
    if (maxd > 58) return fail(ctx, RT_ERR_INTERNAL, "LBVH layout: depth %d exceeds the 58 path bits of the breadth-first sort key", maxd);
    std::vector<int> lvl_off(maxd + 2, 0);
    for (int d = 0; d <= maxd; ++d) lvl_off[d + 1] = lvl_off[d] + hist[d];
    if (lvl_off[maxd + 1] != n_nodes) return fail(ctx, RT_ERR_INTERNAL, "LBVH layout: %d nodes in the depth histogram, %d in the tree", lvl_off[maxd + 1], n_nodes);
    if ((rc = upload(ctx, ctx->lvl_off, lvl_off.data(), lvl_off.size() * sizeof(int))) != RT_OK) return rc;
    ctx->n_levels = maxd + 1;
    rtk::Scene sc = old;
    sc.nrm = nullptr; sc.smooth_mask = 0;
    ctx->n_syn = 0;                                                              // (one mesh: no synthetic nodes)
    sc.n_nodes = n_nodes; sc.n_tris = (int)n;
    mesh_table_single(sc, ctx->parts[0].obj);
    ctx->parts[0].nn = n_nodes;                                                  // (the part's vertex and triangle ranges stay)
    sc.root_lo = root[0]; sc.root_hi = root[1];
    bool fast = true;
    const float rv[6] = {root[0].x, root[0].y, root[0].z, root[1].x, root[1].y, root[1].z};
    float bm[3];
    for (int k = 0; k < 3; ++k) {                                                // every box nests inside the root's (unions, bottom-up), min <= max by construction
        if (!(rv[k] <= rv[k + 3]) || !(std::fabs(rv[k]) < 1e8f) || !(std::fabs(rv[k + 3]) < 1e8f)) fast = false;
        bm[k] = std::max(std::fabs(rv[k]), std::fabs(rv[k + 3]));
    }
    sc.bmx = bm[0]; sc.bmy = bm[1]; sc.bmz = bm[2]; sc.fast_box = fast ? 1 : 0;
    sc.node_lo = static_cast<const float4 *>(ctx->node_lo.p); sc.node_hi = static_cast<const float4 *>(ctx->node_hi.p);
    sc.nodes = static_cast<const float4 *>(ctx->nodes2.p); sc.nodesq = static_cast<const float4 *>(ctx->nodesq.p); sc.nodesb = static_cast<const float4 *>(ctx->nodesb.p);
    sc.q2thr = static_cast<const int *>(ctx->q2thr.p); sc.tri = static_cast<const float4 *>(ctx->tri.p);
    sc.verts = static_cast<const float4 *>(ctx->verts.p); sc.tidx = static_cast<const int4 *>(ctx->tidx.p);
    ctx->travq_ok = n_nodes + 2 < (1 << rtk::kQNodeBits) && (uint64_t)n * 48 < ((uint64_t)1 << 32);   // leaves hold at most kLbvhLeaf triangles
    ctx->scene = sc;
    ctx->host_mesh_stale = true;                                                 // tri_perm / up_indices: on the device now (perm_dev, tidx_up)
    ctx->vcsr_valid = false;                                                     // both orders changed: the adjacency of rt_mesh_compute_normals is rebuilt when next needed,
    ctx->nsnap_mask = 0;                                                         // and a normal snapshot (by visit rank) describes the old layout
    ctx->have_scene = true;
    ctx->q16_topo_ok = true;                                                     // boxes are unions, bottom-up: they nest
    ctx->qw_topo_ok = true;                                                      // (an LBVH leaf holds at least one triangle)
    ctx->q16_leaf_shift = rtk::q16_leaf_shift(rtk::kLbvhLeaf, n);                // leaves of at most kLbvhLeaf triangles
    return requantize(ctx, q);
}

// old_visit[t]: the visit rank, before a rebuild of part P re-laid the scene out, of the triangle now at visit rank t (-1: it had none).  old_perm: tri_perm as it was;
// order: the builder's order of P's triangles (new uploaded index -> old one, both in P's own space); the other parts keep their uploaded order.
static std::vector<int> old_visit_ranks(const rt_ctx *ctx, const std::vector<int> &old_perm, const rt_ctx::MeshPart &P, const std::vector<int> &order) {
    std::vector<int> old_visit_of(ctx->n_up_tris, -1), old_visit(ctx->tri_perm.size());
    for (size_t t = 0; t < old_perm.size(); ++t) old_visit_of[old_perm[t]] = (int)t;
    for (size_t t = 0; t < old_visit.size(); ++t) {
        const int g = ctx->tri_perm[t];
        old_visit[t] = old_visit_of[g >= P.tri_off && g < P.tri_off + P.nt ? P.tri_off + order[g - P.tri_off] : g];
    }
    return old_visit;
}

// A per-corner attribute (smooth normals, UVs) travels with its triangles: new visit rank t takes the three entries of old visit rank old_visit[t], zeros where it had none
// (a template inside the entry points' extern "C" block: C++ linkage said aloud)
extern "C++" template <class T> static std::vector<T> carry_corners(const std::vector<T> &old, const std::vector<int> &old_visit) {
    std::vector<T> out(3 * old_visit.size());                                       // (value-initialised: zeros)
    for (size_t t = 0; t < old_visit.size(); ++t)
        if (old_visit[t] >= 0) for (int k = 0; k < 3; ++k) out[3 * t + k] = old[3 * (size_t)old_visit[t] + k];
    return out;
}

// Part pi rebuilt in `mode` over its triangles (tidx_up + tri_off) and the vertices as they are on the device now; every other part keeps its tree, with the boxes the device
// holds (refitted or as uploaded).  The outputs are in the part's own index space.
static int rebuild_part(rt_ctx *ctx, size_t pi, int mode, float *bvh_arr10_out, int32_t *tri_order_out, int32_t *n_nodes_out) {
    const std::vector<rt_ctx::MeshPart> parts = ctx->parts;
    const rt_ctx::MeshPart P = parts[pi];
    ctx->still.mesh_changed();
    const rtk::Scene old = ctx->scene;
    const int K = (int)parts.size();
    const bool was_valid = ctx->parts_valid;
    if (K > 1 && (ctx->forest_arr.size() != (size_t)old.n_nodes * 10 || ctx->pre_of.size() != (size_t)old.n_nodes))
        return fail(ctx, RT_ERR_INTERNAL, "forest records do not match the tree in use");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t q = own_stream(ctx);
    int rc;
    int n_nodes = 0;
    ctx->build = rt_build_stats{};
    hipEvent_t e0 = ctx->ev_t0, e1 = ctx->ev_t1;                                    // (the tone-mapping events are free here: nothing else runs on the stream)
    RT_HIP(ctx, hipEventRecord(e0, q));
    // a mesh of a single leaf's worth of triangles is a single leaf in either mode (cpu:217: fewer than five triangles are never split)
    if (mode == RT_BVH_LBVH && P.nt > 4) rc = rebuild_lbvh_tree(ctx, P.nt, n_nodes, P.tri_off);
    else { mode = RT_BVH_REFERENCE; rc = rebuild_reference_tree(ctx, P.nt, n_nodes, P.tri_off); }
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipEventRecord(e1, q));
    RT_HIP(ctx, hipEventSynchronize(e1));
    RT_HIP(ctx, hipEventElapsedTime(&ctx->build.device_build_ms, e0, e1));
    ctx->have_tonemap_time = false;                                                 // (the borrowed events no longer bracket a tone mapping)
    ctx->build.mode = mode; ctx->build.n_nodes = n_nodes; ctx->build.n_triangles = P.nt;
    const auto t_install = std::chrono::steady_clock::now();
    int *const order_dev = static_cast<int *>(ctx->bb_idx.p);
    // (normals and UVs travel on the host path; so does a forest: no device-side install of several meshes)
    if (K == 1 && mode == RT_BVH_LBVH && old.nrm == nullptr && ctx->tex_mask == 0 && !ctx->lbvh_host_install && ctx->build.max_depth <= 56) {
        // the kernels' formats straight from the builder's arrays; the flat tree and the order travel to the host only if the caller asks
        if ((rc = install_lbvh_device(ctx, old, n_nodes)) != RT_OK) return rc;
        if (bvh_arr10_out) RT_HIP(ctx, hipMemcpyAsync(bvh_arr10_out, ctx->bb_arr.p, (size_t)n_nodes * 10 * sizeof(float), hipMemcpyDeviceToHost, q));
        if (tri_order_out) RT_HIP(ctx, hipMemcpyAsync(tri_order_out, order_dev, (size_t)P.nt * sizeof(int), hipMemcpyDeviceToHost, q));
        RT_HIP(ctx, hipStreamSynchronize(q));
        if (n_nodes_out) *n_nodes_out = n_nodes;
        ctx->build.install_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_install).count();
        ctx->build.install_on_device = 1;
        return RT_OK;
    }
    if ((rc = refresh_host_mesh(ctx)) != RT_OK) return rc;                          // the host path below starts from up_indices / tri_perm
    // The tree is built.  The O(n) re-layout for the kernels (traversal order, visit-order triangle records, sibling pairs, refit levels) reuses the upload path on the
    // host: ~30 bytes per triangle over PCIe each way.  What the device holds: the new tree and order, every vertex, the normals and UVs, and for a forest every node box.
    std::vector<float> arr((size_t)n_nodes * 10);
    std::vector<int> order(P.nt);
    std::vector<float4> hv(old.n_verts), nlo(K > 1 ? old.n_nodes : 0), nhi(nlo.size()), old_nrm;
    RT_HIP(ctx, hipMemcpyAsync(arr.data(), ctx->bb_arr.p, arr.size() * sizeof(float), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipMemcpyAsync(order.data(), order_dev, order.size() * sizeof(int), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipMemcpyAsync(hv.data(), ctx->verts.p, hv.size() * sizeof(float4), hipMemcpyDeviceToHost, q));
    if (!nlo.empty()) {
        RT_HIP(ctx, hipMemcpyAsync(nlo.data(), ctx->node_lo.p, nlo.size() * sizeof(float4), hipMemcpyDeviceToHost, q));
        RT_HIP(ctx, hipMemcpyAsync(nhi.data(), ctx->node_hi.p, nhi.size() * sizeof(float4), hipMemcpyDeviceToHost, q));
    }
    if (old.nrm != nullptr) {
        old_nrm.resize((size_t)old.n_tris * 3);
        RT_HIP(ctx, hipMemcpyAsync(old_nrm.data(), ctx->nrm.p, old_nrm.size() * sizeof(float4), hipMemcpyDeviceToHost, q));
    }
    RT_HIP(ctx, hipStreamSynchronize(q));
    std::vector<float2> old_uv;
    if (ctx->tex_mask != 0 && old.n_tris > 0) {
        old_uv.resize(3 * (size_t)old.n_tris);
        RT_HIP(ctx, hipMemcpy(old_uv.data(), ctx->tex_uv.p, old_uv.size() * sizeof(float2), hipMemcpyDeviceToHost));
    }
    // every mesh in its own index space, in object order, as rt_scene_upload_meshes receives them
    std::vector<std::vector<float>> vx(K), ar(K);
    std::vector<std::vector<int32_t>> ix(K);
    std::vector<rt_mesh> ms(K);
    std::vector<int> real(K);
    for (int k = 0; k < K; ++k) {
        const rt_ctx::MeshPart &Q = parts[k];
        const bool me = k == (int)pi;
        vx[k].resize((size_t)Q.nv * 3);
        for (int i = 0; i < Q.nv; ++i) { const float4 v = hv[(size_t)Q.voff + i]; vx[k][3 * (size_t)i] = v.x; vx[k][3 * (size_t)i + 1] = v.y; vx[k][3 * (size_t)i + 2] = v.z; }
        ix[k].resize((size_t)Q.nt * 3);
        for (int t = 0; t < Q.nt; ++t) {
            const int src = me ? order[t] : t;                                      // the rebuilt mesh: its triangles in the builder's order
            for (int c = 0; c < 3; ++c) ix[k][3 * (size_t)t + c] = ctx->up_indices[3 * ((size_t)Q.tri_off + src) + c] - Q.voff;
        }
        if (!me) {                                                                  // its tree as installed, the boxes the device holds now
            ar[k].resize((size_t)Q.nn * 10);
            for (int n = 0; n < Q.nn; ++n) {
                const float *a = ctx->forest_arr.data() + ((size_t)Q.noff + n) * 10;
                float *o = ar[k].data() + (size_t)n * 10;
                const int x = ctx->pre_of[(size_t)Q.noff + n];
                o[0] = a[0] == -1.f ? -1.f : (float)((int)a[0] - Q.noff); o[1] = a[1] == -1.f ? -1.f : (float)((int)a[1] - Q.noff);
                o[2] = nlo[x].x; o[3] = nlo[x].y; o[4] = nlo[x].z; o[5] = nhi[x].x; o[6] = nhi[x].y; o[7] = nhi[x].z;
                o[8] = (float)((int)a[8] - Q.tri_off); o[9] = (float)((int)a[9] - Q.tri_off);
            }
        }
        rt_mesh &m = ms[k];
        m = rt_mesh{};
        m.vertices = vx[k].data(); m.n_vertices = Q.nv; m.indices = ix[k].data(); m.index_stride = 3; m.n_triangles = Q.nt;
        m.bvh_arr10 = me ? arr.data() : ar[k].data(); m.n_nodes = me ? n_nodes : Q.nn;
        m.object_slot = Q.obj;                                                      // (albedo and material stay in the scene's mesh table, which `sc` carries over)
        real[k] = k;
    }
    const std::vector<int> old_perm = ctx->tri_perm;                               // old visit order -> old uploaded order
    rtk::Scene sc = old;
    sc.n_nodes = sc.n_tris = sc.n_verts = 0; sc.nrm = nullptr;
    if ((rc = install_meshes(ctx, sc, ms.data(), real)) != RT_OK) return rc;
    ctx->parts_valid = was_valid;                                                   // (a plain rebuild after a failed upload does not make the *_of entries answer again)
    for (int k = 0; k < K; ++k) ctx->parts[k].smooth = parts[k].smooth;            // ranges keep their sizes; the rebuilt mesh's node count changed
    if (!old_nrm.empty() || !old_uv.empty()) {                                     // smooth normals and UVs travel with their triangles, every mesh's
        const std::vector<int> old_visit = old_visit_ranks(ctx, old_perm, P, order);
        if (!old_nrm.empty()) {
            const std::vector<float4> nn = carry_corners(old_nrm, old_visit);
            if ((rc = upload(ctx, ctx->nrm, nn.data(), nn.size() * sizeof(float4))) != RT_OK) return rc;
            ctx->scene.nrm = static_cast<const float4 *>(ctx->nrm.p);
        }
        if (!old_uv.empty()) {
            const std::vector<float2> nu = carry_corners(old_uv, old_visit);
            if ((rc = upload(ctx, ctx->tex_uv, nu.data(), nu.size() * sizeof(float2))) != RT_OK) return rc;
        }
    }
    if (bvh_arr10_out) memcpy(bvh_arr10_out, arr.data(), arr.size() * sizeof(float));
    if (tri_order_out) memcpy(tri_order_out, order.data(), order.size() * sizeof(int));
    if (n_nodes_out) *n_nodes_out = n_nodes;
    ctx->build.install_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_install).count();
    return RT_OK;
}

int rt_mesh_rebuild_mode(rt_ctx *ctx, int mode, float *bvh_arr10_out, int32_t *tri_order_out, int32_t *n_nodes_out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (mode != RT_BVH_REFERENCE && mode != RT_BVH_LBVH) return fail(ctx, RT_ERR_INVALID, "unknown BVH mode %d", mode);
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (n_nodes_out) *n_nodes_out = 0;
    if (ctx->parts.size() > 1) return fail(ctx, RT_ERR_UNSUPPORTED, "the scene holds %d meshes: a rebuild works on ONE TriangleMesh (upload the rebuilt meshes again)", (int)ctx->parts.size());
    if (ctx->parts.empty()) return RT_OK;                                           // no mesh: nothing to build
    return rebuild_part(ctx, 0, mode, bvh_arr10_out, tri_order_out, n_nodes_out);
}

int rt_mesh_rebuild(rt_ctx *ctx, float *bvh_arr10_out, int32_t *tri_order_out, int32_t *n_nodes_out) {
    return rt_mesh_rebuild_mode(ctx, RT_BVH_REFERENCE, bvh_arr10_out, tri_order_out, n_nodes_out);
}

int rt_mesh_rebuild_of(rt_ctx *ctx, int object_slot, int mode, float *bvh_arr10_out, int32_t *tri_order_out, int32_t *n_nodes_out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (mode != RT_BVH_REFERENCE && mode != RT_BVH_LBVH) return fail(ctx, RT_ERR_INVALID, "unknown BVH mode %d", mode);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    if (n_nodes_out) *n_nodes_out = 0;
    if (!p) return RT_OK;                                                           // a mesh without triangles: nothing to build
    return rebuild_part(ctx, p - ctx->parts.data(), mode, bvh_arr10_out, tri_order_out, n_nodes_out);
}

int rt_mesh_build_stats(const rt_ctx *ctx, rt_build_stats *out) {
    if (!ctx || !out) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    *out = ctx->build;
    return RT_OK;
}
