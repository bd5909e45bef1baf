// dsr_mesh_indexed.hip — the indexed mesh of the map: vertices[] + indices[] with per-vertex normals and colours
// (include/dsr_mesh.h "indexed meshes"; builder-defined).
//
// The entry points: flags and arguments, the read-backs, the PLY and OBJ writers.  Host code only — the kernels (k_mesh_indexed.h)
// build on the soup mesher's source policies and scans, whose one includer is dsr_engine.hip, so the launches live there
// (dsr_internal::engine_mesh_indexed) and fill dsr_engine::imesh, the slot this file serves.
#include "dsr_internal.h"

using namespace dsr_internal;

namespace {

constexpr int kKnownFlags = DSR_MESH_COMPLETE | DSR_MESH_COLOURS | DSR_MESH_NORMALS;

// elements first .. first + count - 1 of a device array of `words` 4-byte words per element
int read_back(dsr_engine *e, void *out, const void *dev, int words, uint64_t have, uint64_t first, uint64_t count, const char *what) {
  if (!e->imesh.valid) return fail(DSR_E_ARG, "no indexed mesh (dsr_mesh_scene_indexed makes one)");
  if (!out && count) return fail(DSR_E_ARG, "null");
  if (first > have || count > have - first) return fail(DSR_E_ARG, std::string(what) + " range outside the indexed mesh");
  if (count) {
    HIP_TRY(hipMemcpyAsync(out, static_cast<const uint8_t *>(dev) + (size_t)first * words * 4, (size_t)count * words * 4,
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return DSR_OK;
}

bool ends_in_ply(const char *path) {
  const size_t n = strlen(path);
  return n >= 4 && path[n - 4] == '.' && (path[n - 3] | 0x20) == 'p' && (path[n - 2] | 0x20) == 'l' && (path[n - 1] | 0x20) == 'y';
}

// the whole mesh on the host (the writers; a file is written by one pass over each array)
struct HostMesh {
  std::vector<float> verts, normals;
  std::vector<uint8_t> colours;
  std::vector<uint32_t> indices;
  bool hasNormals = false, hasColours = false;
  uint64_t nv = 0, nt = 0;
};
int fetch(dsr_engine *e, HostMesh &h) {
  const dsr_engine::IndexedMesh &m = e->imesh;
  if (!m.valid) return fail(DSR_E_ARG, "no indexed mesh (dsr_mesh_scene_indexed makes one)");
  h.nv = m.nVerts; h.nt = m.nTris;
  h.hasNormals = (m.flags & DSR_MESH_NORMALS) != 0; h.hasColours = (m.flags & DSR_MESH_COLOURS) != 0;
  int st;
  h.verts.resize((size_t)h.nv * 3); h.indices.resize((size_t)h.nt * 3);
  if ((st = dsr_mesh_indexed_get_vertices(e, h.verts.data(), 0, h.nv)) || (st = dsr_mesh_indexed_get_indices(e, h.indices.data(), 0, h.nt)))
    return st;
  if (h.hasNormals) {
    h.normals.resize((size_t)h.nv * 3);
    if ((st = dsr_mesh_indexed_get_normals(e, h.normals.data(), 0, h.nv))) return st;
  }
  if (h.hasColours) {
    h.colours.resize((size_t)h.nv * 4);
    if ((st = dsr_mesh_indexed_get_colours(e, h.colours.data(), 0, h.nv))) return st;
  }
  return DSR_OK;
}

}  // namespace

extern "C" {

int32_t dsr_mesh_indexed_abi_version(void) { return DSR_MESH_INDEXED_ABI_VERSION; }

int dsr_mesh_scene_indexed(dsr_engine *e, int flags, uint64_t *n_vertices, uint64_t *n_triangles) {
  // (with DSR_MESH_COMPLETE no deferred render is queued, as in dsr_mesh_scene_complete: it reads the scene, as this call does)
  if (e && (flags & DSR_MESH_COMPLETE)) { CHECK_E_NOFLUSH(e); }
  else { CHECK_E(e); }
  if (n_vertices) *n_vertices = 0;
  if (n_triangles) *n_triangles = 0;
  if (flags & ~kKnownFlags) return fail(DSR_E_ARG, "unknown flag (DSR_MESH_COMPLETE, DSR_MESH_COLOURS, DSR_MESH_NORMALS)");
  const int st = engine_mesh_indexed(e, flags);
  if (st == DSR_OK) {
    if (n_vertices) *n_vertices = e->imesh.nVerts;
    if (n_triangles) *n_triangles = e->imesh.nTris;
  }
  return st;
}

int dsr_mesh_indexed_get_vertices(dsr_engine *e, float *xyz, uint64_t first, uint64_t count) {
  CHECK_E(e);
  return read_back(e, xyz, e->imesh.verts, 3, e->imesh.nVerts, first, count, "vertex");
}

int dsr_mesh_indexed_get_normals(dsr_engine *e, float *xyz, uint64_t first, uint64_t count) {
  CHECK_E(e);
  if (e->imesh.valid && !(e->imesh.flags & DSR_MESH_NORMALS))
    return fail(DSR_E_ARG, "the indexed mesh has no normals (DSR_MESH_NORMALS makes one that has)");
  return read_back(e, xyz, e->imesh.normals, 3, e->imesh.nVerts, first, count, "vertex");
}

int dsr_mesh_indexed_get_colours(dsr_engine *e, uint8_t *rgba, uint64_t first, uint64_t count) {
  CHECK_E(e);
  if (e->imesh.valid && !(e->imesh.flags & DSR_MESH_COLOURS))
    return fail(DSR_E_ARG, "the indexed mesh has no colours (DSR_MESH_COLOURS makes one that has)");
  return read_back(e, rgba, e->imesh.colours, 1, e->imesh.nVerts, first, count, "vertex");
}

int dsr_mesh_indexed_get_indices(dsr_engine *e, uint32_t *out, uint64_t first_triangle, uint64_t count) {
  CHECK_E(e);
  return read_back(e, out, e->imesh.indices, 3, e->imesh.nTris, first_triangle, count, "triangle");
}

int dsr_mesh_indexed_free(dsr_engine *e) {
  CHECK_E(e);
  return engine_mesh_indexed_release(e);
}

int dsr_mesh_indexed_write_ply(dsr_engine *e, const char *path) {
  CHECK_E(e);
  if (!path) return fail(DSR_E_ARG, "null path");
  HostMesh h;
  int st = fetch(e, h);
  if (st) return st;
  if (h.nv > 0x7fffffffull) return fail(DSR_E_ARG, "too many vertices for the int indices of a PLY face");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(DSR_E_ARG, "cannot open the PLY file for writing");
  fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %llu\nproperty float x\nproperty float y\nproperty float z\n",
          (unsigned long long)h.nv);
  if (h.hasNormals) fprintf(f, "property float nx\nproperty float ny\nproperty float nz\n");
  if (h.hasColours) fprintf(f, "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n");
  fprintf(f, "element face %llu\nproperty list uchar int vertex_indices\nend_header\n", (unsigned long long)h.nt);
  const size_t vb = 12 + (h.hasNormals ? 12 : 0) + (h.hasColours ? 4 : 0);
  const uint64_t chunk = 1u << 16;
  std::vector<uint8_t> rec((size_t)chunk * std::max<size_t>(vb, 13));
  for (uint64_t first = 0; first < h.nv; first += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, h.nv - first);
    for (uint64_t i = 0; i < cnt; ++i) {
      uint8_t *o = rec.data() + (size_t)i * vb;
      memcpy(o, &h.verts[(size_t)(first + i) * 3], 12); o += 12;
      if (h.hasNormals) { memcpy(o, &h.normals[(size_t)(first + i) * 3], 12); o += 12; }
      if (h.hasColours) memcpy(o, &h.colours[(size_t)(first + i) * 4], 4);
    }
    fwrite(rec.data(), 1, (size_t)cnt * vb, f);
  }
  for (uint64_t first = 0; first < h.nt; first += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, h.nt - first);
    for (uint64_t i = 0; i < cnt; ++i) {
      uint8_t *o = rec.data() + (size_t)i * 13;
      const uint32_t *t = &h.indices[(size_t)(first + i) * 3];
      const int32_t idx[3] = {(int32_t)t[2], (int32_t)t[1], (int32_t)t[0]};
      o[0] = 3;
      memcpy(o + 1, idx, 12);
    }
    fwrite(rec.data(), 1, (size_t)cnt * 13, f);
  }
  const bool bad = ferror(f) != 0;
  if (fclose(f) != 0 || bad) return fail(DSR_E_ARG, "writing the PLY file failed");
  return DSR_OK;
}

int dsr_mesh_indexed_write_obj(dsr_engine *e, const char *path) {
  CHECK_E(e);
  if (!path) return fail(DSR_E_ARG, "null path");
  HostMesh h;
  int st = fetch(e, h);
  if (st) return st;
  FILE *f = fopen(path, "w+");
  if (!f) return fail(DSR_E_ARG, "cannot open the OBJ file for writing");
  for (uint64_t i = 0; i < h.nv; ++i) {
    const float *p = &h.verts[(size_t)i * 3];
    if (h.hasColours) {
      const uint8_t *c = &h.colours[(size_t)i * 4];
      fprintf(f, "v %f %f %f %f %f %f\n", p[0], p[1], p[2], (float)c[0] / 255.0f, (float)c[1] / 255.0f, (float)c[2] / 255.0f);
    } else {
      fprintf(f, "v %f %f %f\n", p[0], p[1], p[2]);
    }
  }
  for (uint64_t i = 0; h.hasNormals && i < h.nv; ++i) {
    const float *q = &h.normals[(size_t)i * 3];
    fprintf(f, "vn %f %f %f\n", q[0], q[1], q[2]);
  }
  for (uint64_t i = 0; i < h.nt; ++i) {
    const uint32_t *t = &h.indices[(size_t)i * 3];
    const unsigned long long a = (unsigned long long)t[2] + 1, b = (unsigned long long)t[1] + 1, c = (unsigned long long)t[0] + 1;
    if (h.hasNormals) fprintf(f, "f %llu//%llu %llu//%llu %llu//%llu\n", a, a, b, b, c, c);
    else fprintf(f, "f %llu %llu %llu\n", a, b, c);
  }
  const bool bad = ferror(f) != 0;
  if (fclose(f) != 0 || bad) return fail(DSR_E_ARG, "writing the OBJ file failed");
  return DSR_OK;
}

int dsr_save_scene_to_mesh_indexed(dsr_engine *e, const char *path, int flags) {
  if (e && !path) return fail(DSR_E_ARG, "null path");
  int st = dsr_mesh_scene_indexed(e, flags, nullptr, nullptr);
  if (st == DSR_OK) st = ends_in_ply(path) ? dsr_mesh_indexed_write_ply(e, path) : dsr_mesh_indexed_write_obj(e, path);
  if (e) (void)engine_mesh_indexed_release(e);
  return st;
}

}  // extern "C"
