// rt_host_tex.hip.h -- host side (inside rt_capi.hip's extern "C" block): textured meshes.  rt_mesh_set_texture[_of] store a mesh's per-corner UVs in visit order
// (as rt_mesh_set_normals[_of] store normals), its texels as 8-bit bytes and its decode table on the device, and set its bit in tex_mask: frames then run
// wf_advance<kFormTex> (rt_wavefront.hip.h).  rt_mesh_rebuild* carry the UVs with their triangles (rt_host_mesh.hip.h, which also has the gather both share); rt_mesh_transform* leave them alone.
#pragma once

static_assert(rtk::kMaxObjects == RT_MAX_OBJECTS, "the texture table is indexed by object id");

int rt_mesh_set_texture_of(rt_ctx *ctx, int object_slot, const float *uvs, int n_uvs, const int32_t *uvidx, int index_stride, int n_triangles, const rt_texture *tex) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    rt_ctx::MeshPart *p = nullptr;
    if (int rc = find_part(ctx, object_slot, p); rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipDeviceSynchronize());                                            // frames in flight may read the records and buffers replaced below
    ctx->still.shading_changed();
    const int bit = 1 << object_slot;
    if (!uvs || !uvidx || !tex) {                                                   // this mesh untextured again
        ctx->tex_mask &= ~bit;
        return RT_OK;
    }
    if (n_uvs <= 0 || index_stride < 3) return fail(ctx, RT_ERR_INVALID, "bad UV array sizes");
    if (tex->width <= 0 || tex->height <= 0) return fail(ctx, RT_ERR_INVALID, "texture size %d x %d", tex->width, tex->height);
    if (tex->channels != 3 && tex->channels != 4) return fail(ctx, RT_ERR_INVALID, "a texel has 3 or 4 bytes, not %d", tex->channels);
    if (tex->filter != RT_TEX_NEAREST && tex->filter != RT_TEX_BILINEAR) return fail(ctx, RT_ERR_INVALID, "unknown texture filter %d", tex->filter);
    if (tex->wrap != RT_TEX_REPEAT && tex->wrap != RT_TEX_CLAMP) return fail(ctx, RT_ERR_INVALID, "unknown texture wrap mode %d", tex->wrap);
    if (!tex->texels) return fail(ctx, RT_ERR_INVALID, "texels is NULL");
    const size_t n_texels = (size_t)tex->width * (size_t)tex->height;
    if (n_texels >= ((size_t)1 << 31) / 4) return fail(ctx, RT_ERR_INVALID, "texture of %d x %d texels: at most 2^29 texels", tex->width, tex->height);
    if (!p) return RT_OK;                                                           // a mesh without triangles: never hit, nothing to texture
    const rtk::Scene &sc = ctx->scene;
    int vb, rc;
    std::vector<int> ui;
    if ((rc = gather_corners(ctx, *p, "UV", uvidx, index_stride, n_triangles, n_uvs, vb, ui)) != RT_OK) return rc;
    std::vector<float2> uv(ui.size());
    for (size_t i = 0; i < ui.size(); ++i) uv[i] = make_float2(uvs[2 * (size_t)ui[i]], uvs[2 * (size_t)ui[i] + 1]);
    // the decode table (NULL: byte / 255, one correctly rounded division) and the texels, one buffer per object
    std::vector<uint8_t> img(1024 + n_texels * tex->channels);
    float *dec = reinterpret_cast<float *>(img.data());
    for (int b = 0; b < 256; ++b) dec[b] = tex->decode ? tex->decode[b] : (float)b / 255.0f;
    memcpy(img.data() + 1024, tex->texels, n_texels * tex->channels);
    if ((rc = ensure(ctx, ctx->tex_uv, 3 * (size_t)std::max(sc.n_tris, 1) * sizeof(float2))) != RT_OK) return rc;
    if ((rc = upload(ctx, ctx->tex_img[object_slot], img.data(), img.size())) != RT_OK) return rc;
    if (!uv.empty()) RT_HIP(ctx, hipMemcpy(static_cast<float2 *>(ctx->tex_uv.p) + 3 * (size_t)vb, uv.data(), uv.size() * sizeof(float2), hipMemcpyHostToDevice));
    rtk::TexDesc &d = ctx->tex_desc[object_slot];
    d.decode = static_cast<const float *>(ctx->tex_img[object_slot].p);
    d.texels = static_cast<const uint8_t *>(ctx->tex_img[object_slot].p) + 1024;
    d.w = tex->width; d.h = tex->height; d.ch = tex->channels; d.filter = tex->filter; d.wrap = tex->wrap; d.pad = 0;
    if ((rc = upload(ctx, ctx->tex_table, ctx->tex_desc, sizeof(ctx->tex_desc))) != RT_OK) return rc;
    ctx->tex_mask |= bit;
    return RT_OK;
}

int rt_mesh_set_texture(rt_ctx *ctx, const float *uvs, int n_uvs, const int32_t *uvidx, int index_stride, int n_triangles, const rt_texture *tex) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    if (!uvs || !uvidx || !tex) {                                                   // every mesh untextured again
        ctx->still.shading_changed();
        ctx->tex_mask = 0;
        return RT_OK;
    }
    if (ctx->parts.size() > 1) return fail(ctx, RT_ERR_UNSUPPORTED, "the scene holds %d meshes: a texture is set for ONE TriangleMesh (rt_mesh_set_texture_of)", (int)ctx->parts.size());
    if (ctx->parts.empty()) return fail(ctx, RT_ERR_INVALID, "the scene has no mesh");
    return rt_mesh_set_texture_of(ctx, ctx->parts[0].obj, uvs, n_uvs, uvidx, index_stride, n_triangles, tex);
}
