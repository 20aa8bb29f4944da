// vrhip/IsoMesh.hpp -- the iso-surface of a dense volume as an indexed triangle mesh, from C++: IsoMesher counts,
// allocates and emits (vr_isomesh_workspace_bytes / vr_isomesh_count / vr_isomesh_emit) and owns its workspace; Mesh is
// the host copy.  The rule is in vrhip.h ("iso-surface meshes").  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace vrhip {

// positions / gradients: 3 floats per vertex (voxel-centre index coordinates; gradients empty unless asked for);
// indices: 3 per triangle, counter-clockwise seen from the outside
struct Mesh {
    std::vector<float> positions, gradients;
    std::vector<uint32_t> indices;
    size_t num_vertices() const { return positions.size() / 3; }
    size_t num_triangles() const { return indices.size() / 3; }
};

class IsoMesher {
public:
    IsoMesher() = default;
    IsoMesher(const IsoMesher &) = delete;
    IsoMesher &operator=(const IsoMesher &) = delete;
    ~IsoMesher() { release(); }

    // The desc of the whole of a volume of `dims` voxels held in full: every cell, the cap's outer layer included.
    static vr_isomesh_desc whole(const int64_t dims[3], float iso_value, bool cap)
    {
        vr_isomesh_desc d{};
        d.iso_value = iso_value;
        d.cap = cap ? 1 : 0;
        for (int k = 0; k < 3; ++k) {
            d.global_dims[k] = dims[k];
            d.vol_origin[k] = 0;
            d.own_lo[k] = cap ? -1 : 0;
            d.own_hi[k] = cap ? dims[k] : dims[k] - 1;
        }
        return d;
    }

    // Counts the mesh of `desc` over volume_dev (the voxels [vol_origin, vol_origin + dims)); the workspace is kept
    // for emit().  Synchronises `stream`.
    void count(const uint8_t *volume_dev, const int64_t dims[3], const vr_isomesh_desc &desc, void *stream = nullptr)
    {
        int64_t bytes = 0;
        check(vr_isomesh_workspace_bytes(dims, &desc, &bytes), "vr_isomesh_workspace_bytes");
        if (bytes > capacity_) {
            release();
            check(vr_malloc(&workspace_, bytes), "vr_malloc");
            capacity_ = bytes;
        }
        counted_ = false;
        uint64_t c[2] = {0, 0};
        check(vr_isomesh_count(volume_dev, dims, &desc, workspace_, c, stream), "vr_isomesh_count");
        vertices_ = c[0]; triangles_ = c[1];
        volume_ = volume_dev; desc_ = desc;
        for (int k = 0; k < 3; ++k) dims_[k] = dims[k];
        counted_ = true;
    }
    uint64_t num_vertices() const { return vertices_; }
    uint64_t num_triangles() const { return triangles_; }

    // Emits what count() counted into the caller's device buffers: 3 floats per vertex, 3 uint32 per triangle;
    // gradients_dev may be null.  Asynchronous on `stream`.
    void emit(float *positions_dev, float *gradients_dev, uint32_t *indices_dev, void *stream = nullptr) const
    {
        if (!counted_) throw std::logic_error("IsoMesher::emit before count");
        check(vr_isomesh_emit(volume_, dims_, &desc_, workspace_, (int64_t)vertices_, (int64_t)triangles_, positions_dev,
                              gradients_dev, indices_dev, stream), "vr_isomesh_emit");
    }

    // count + allocate + emit + download
    Mesh extract(const uint8_t *volume_dev, const int64_t dims[3], const vr_isomesh_desc &desc, bool gradients = false,
                 void *stream = nullptr)
    {
        count(volume_dev, dims, desc, stream);
        Mesh m;
        m.positions.resize((size_t)vertices_ * 3);
        if (gradients) m.gradients.resize((size_t)vertices_ * 3);
        m.indices.resize((size_t)triangles_ * 3);
        if (vertices_ == 0 && triangles_ == 0) return m;
        const int64_t vb = (int64_t)vertices_ * 12, tb = (int64_t)triangles_ * 12;
        Buffer pos(vb), grad(gradients ? vb : 0), idx(tb);
        emit((float *)pos.p, (float *)grad.p, (uint32_t *)idx.p, stream);
        check(vr_download(m.positions.data(), pos.p, vb, stream), "vr_download");
        if (gradients) check(vr_download(m.gradients.data(), grad.p, vb, stream), "vr_download");
        check(vr_download(m.indices.data(), idx.p, tb, stream), "vr_download");
        return m;
    }

private:
    struct Buffer {
        void *p = nullptr;
        explicit Buffer(int64_t bytes) { if (bytes > 0) check(vr_malloc(&p, bytes), "vr_malloc"); }
        Buffer(const Buffer &) = delete;
        Buffer &operator=(const Buffer &) = delete;
        ~Buffer() { if (p) vr_free(p); }
    };
    static void check(vr_status s, const char *what)
    {
        if (s != VR_OK) throw std::runtime_error(std::string(what) + ": " + vr_status_string(s));
    }
    void release()
    {
        if (workspace_) vr_free(workspace_);
        workspace_ = nullptr; capacity_ = 0; counted_ = false;
    }

    void *workspace_ = nullptr;
    int64_t capacity_ = 0;
    bool counted_ = false;
    uint64_t vertices_ = 0, triangles_ = 0;
    const uint8_t *volume_ = nullptr;
    int64_t dims_[3] = {0, 0, 0};
    vr_isomesh_desc desc_{};
};

// A Mesh as a binary little-endian PLY (x y z per vertex, a uchar 3 and three uint indices per face); false if the
// file cannot be written.  For little-endian hosts.
inline bool write_ply(const std::string &path, const Mesh &m)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment vrhip iso-surface mesh\nelement vertex %zu\n"
                    "property float x\nproperty float y\nproperty float z\nelement face %zu\n"
                    "property list uchar uint vertex_indices\nend_header\n", m.num_vertices(), m.num_triangles());
    bool ok = m.positions.empty() || std::fwrite(m.positions.data(), 4, m.positions.size(), f) == m.positions.size();
    for (size_t t = 0; ok && t < m.num_triangles(); ++t) {
        const unsigned char three = 3;
        ok = std::fwrite(&three, 1, 1, f) == 1 && std::fwrite(&m.indices[3 * t], 4, 3, f) == 3;
    }
    return std::fclose(f) == 0 && ok;
}

} // namespace vrhip
