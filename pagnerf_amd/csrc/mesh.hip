// Panoptic surface-mesh export: SURFACE NETS on the density lattice (pagnerf_amd/mesh.py: surface_nets_reference is the definition).
//
// field f32 [nx, ny, nz] (z fastest) and an iso value: a lattice point is INSIDE when v >= iso (a NaN is outside); a cell is ACTIVE when its 8 corners
// are finite and neither all inside nor all outside.  Every active cell owns one vertex, every sign-changing lattice edge whose four cells have a
// vertex one quad.  Both are an ORDERED APPEND (ordered_append.h: count, scan and write pass, three launches, no host synchronisation):
//   pag_mesh_vertices  a row is a cell (linear order, x slowest), MeshCellPred the predicate; the write pass forms the vertex and the normal of the
//                      kept cells and stores every cell's slot (-1 for a cell without vertex) into cell_vertex
//   pag_mesh_faces     a row is r = point * 3 + axis, the lattice edge from P to P + e_axis, MeshEdgePred the predicate (it reads the field at the
//                      two ends and cell_vertex at the four cells around the edge); the write pass stores the quad's two triangles
// so vertex and face order do not depend on the launch geometry.  Neighbouring threads run along z: a workgroup of the cell pass reads the four
// z-rows of its cells coalesced, and the reuse of a row by the neighbouring cells in y and x is left to L2 / MALL.  The 8 corners and 12 edges are
// unrolled straight-line code on registers (no scratch).  fp32 in the definition's op order; compiled with -ffp-contract=off, and division and
// square root are the correctly rounded ones, so vertices and normals are the definition's bits.  Integer and fp32 work only, no atomics.
#include "ordered_append.h"

namespace {

// corner c of a cell = bx * 4 + by * 2 + bz; the 12 edges axis-major, the two other axes' bits (bu, bv) = 00, 01, 10, 11 with the lower axis slower
__device__ __forceinline__ constexpr int mesh_shift(int axis) { return 2 - axis; }
__device__ __forceinline__ constexpr int mesh_edge_a(int a, int e) {
    const int u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
    return (((e >> 1) & 1) << mesh_shift(u)) | ((e & 1) << mesh_shift(v));
}

template <class T>
__device__ __forceinline__ T mesh_pick(uint32_t a, T x0, T x1, T x2) { return a == 0 ? x0 : (a == 1 ? x1 : x2); }

struct MeshCellPred {
    int64_t n;                      // cells
    const float *field;
    uint32_t cy, cz;                // cells along y and z
    int64_t sx, sy;                 // the field's strides of x and y in elements (ny * nz, nz)
    float iso;
    // the cell's indices and corners; -> active.  An out-of-range row reads nothing.
    __device__ __forceinline__ bool corners(int64_t i, uint32_t &ci, uint32_t &cj, uint32_t &ck, float (&v)[8]) const {
        if (i >= n) return false;
        uint32_t q = (uint32_t)i;
        ck = q % cz;
        q /= cz;
        cj = q % cy;
        ci = q / cy;
        const float *p = field + ((int64_t)ci * sx + (int64_t)cj * sy + ck);
        v[0] = p[0], v[1] = p[1], v[2] = p[sy], v[3] = p[sy + 1];
        v[4] = p[sx], v[5] = p[sx + 1], v[6] = p[sx + sy], v[7] = p[sx + sy + 1];
        bool finite = true;
        int inside = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            finite = finite && fabsf(v[c]) <= 3.402823466e38f;          // false for inf and NaN
            inside += v[c] >= iso ? 1 : 0;
        }
        return finite && inside != 0 && inside != 8;
    }
    __device__ __forceinline__ bool operator()(int64_t i) const {
        uint32_t ci, cj, ck;
        float v[8];
        return corners(i, ci, cj, ck, v);
    }
};

struct MeshVertexWrite {
    float lo[3], h;
    int32_t index0[3];
    float *vertices, *normals;
    int32_t *cell_vertex;
    int64_t cap;
};

__global__ __launch_bounds__(OA_BLOCK) void mesh_vertex_write_kernel(MeshCellPred p, MeshVertexWrite w, const int64_t *__restrict__ block_offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    uint32_t cell[3] = {0, 0, 0};
    float v[8];
    const bool keep = p.corners(i, cell[0], cell[1], cell[2], v);
    __shared__ int wc[OA_WAVES];
    const OaVote vote = oa_vote(keep);
    if (lane == 0) wc[wave] = vote.wcount;
    __syncthreads();
    const int64_t dst = oa_wave_base(block_offset, wc) + vote.rank;
    if (i < p.n) w.cell_vertex[i] = keep ? (int32_t)dst : -1;
    if (!keep || dst >= w.cap) return;
    float S[3] = {0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};
    int crossings = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int A = mesh_edge_a(a, e), B = A | (1 << mesh_shift(a));
            const float vA = v[A], vB = v[B];
            const bool cross = (vA >= p.iso) != (vB >= p.iso);
            const float d = vB - vA;
            const float t = (p.iso - vA) / d;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const float comp = x == a ? t : (float)((A >> mesh_shift(x)) & 1);
                S[x] = S[x] + (cross ? comp : 0.0f);
            }
            crossings += cross ? 1 : 0;
            g[a] = e == 0 ? d : g[a] + d;
        }
    }
    const float fn = (float)crossings;
    const float m = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const float local = S[x] / fn;
        w.vertices[dst * 3 + x] = ((float)(w.index0[x] + (int32_t)cell[x]) + local) * w.h + w.lo[x];
        w.normals[dst * 3 + x] = m == 0.0f ? 0.0f : -g[x] / m;
    }
}

struct MeshEdgePred {
    int64_t n;                      // edge rows: points * 3
    const float *field;
    const int32_t *cell_vertex;
    uint32_t nx, ny, nz;
    float iso;
    // the quad of row i: q[0..3] the four cells' vertices in the definition's order (already reversed when P is outside); -> kept
    __device__ __forceinline__ bool quad(int64_t i, int32_t (&q)[4]) const {
        if (i >= n) return false;
        const uint32_t pt = (uint32_t)(i / 3), a = (uint32_t)(i - (int64_t)pt * 3);
        uint32_t r = pt;
        const uint32_t pz = r % nz;
        r /= nz;
        const uint32_t py = r % ny, px = r / ny;
        // the axes (a, u, v) = (a, (a + 1) % 3, (a + 2) % 3) picked by selects: an array indexed by `a` would live in scratch
        const uint32_t Pa = mesh_pick(a, px, py, pz), Pu = mesh_pick(a, py, pz, px), Pv = mesh_pick(a, pz, px, py);
        const uint32_t na = mesh_pick(a, nx, ny, nz), nu = mesh_pick(a, ny, nz, nx), nv = mesh_pick(a, nz, nx, ny);
        // the edge and its four cells exist
        if (Pa + 1 >= na || Pu < 1 || Pu + 1 >= nu || Pv < 1 || Pv + 1 >= nv) return false;
        const int64_t sx = (int64_t)ny * nz, sy = nz;
        const bool in_p = field[pt] >= iso;
        if (in_p == (field[(int64_t)pt + mesh_pick(a, sx, sy, (int64_t)1)] >= iso)) return false;
        const int64_t cx = (int64_t)(ny - 1) * (nz - 1), cy = nz - 1;
        const int64_t cu = mesh_pick(a, cy, (int64_t)1, cx), cv = mesh_pick(a, (int64_t)1, cx, cy);
        const int64_t c = (int64_t)px * cx + (int64_t)py * cy + pz;
        const int32_t q0 = cell_vertex[c - cu - cv], q1 = cell_vertex[c - cv], q2 = cell_vertex[c], q3 = cell_vertex[c - cu];
        if (q0 < 0 || q1 < 0 || q2 < 0 || q3 < 0) return false;
        q[0] = in_p ? q0 : q3, q[1] = in_p ? q1 : q2, q[2] = in_p ? q2 : q1, q[3] = in_p ? q3 : q0;
        return true;
    }
    __device__ __forceinline__ bool operator()(int64_t i) const {
        int32_t q[4];
        return quad(i, q);
    }
};

// faces i32 [cap, 3]: the s-th kept row's triangles at rows 2s and 2s + 1; a quad that does not fit whole is counted and not written
__global__ __launch_bounds__(OA_BLOCK) void mesh_face_write_kernel(MeshEdgePred p, int32_t *__restrict__ faces, int64_t cap,
                                                                   const int64_t *__restrict__ block_offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    int32_t q[4] = {0, 0, 0, 0};
    const bool keep = p.quad(i, q);
    __shared__ int wc[OA_WAVES];
    const OaVote vote = oa_vote(keep);
    if (lane == 0) wc[wave] = vote.wcount;
    __syncthreads();
    const int64_t dst = oa_wave_base(block_offset, wc) + vote.rank;
    if (!keep || 2 * dst + 2 > cap) return;
    int32_t *f = faces + dst * 6;
    f[0] = q[0], f[1] = q[1], f[2] = q[2];
    f[3] = q[0], f[4] = q[2], f[5] = q[3];
}

constexpr int64_t MESH_MAX_CELLS = (int64_t)1 << 31;       // vertex ids are i32
constexpr int64_t MESH_MAX_ROWS = (int64_t)1 << 32;        // one thread per edge row, and a launch holds fewer than 2^32 threads

// -> the edge rows of the lattice, 0 for a lattice the kernels do not take (an axis below 2, 2^31 cells or 2^32 edge rows and more)
int64_t mesh_rows(int64_t nx, int64_t ny, int64_t nz) {
    const int64_t lim = MESH_MAX_CELLS;
    if (nx < 2 || ny < 2 || nz < 2 || nx >= lim || ny >= lim || nz >= lim) return 0;
    if ((nx - 1) * (ny - 1) >= lim || (nx - 1) * (ny - 1) * (nz - 1) >= lim) return 0;                            // each product < 2^62
    if (nx * ny >= lim || nx * ny * nz >= lim || nx * ny * nz * 3 >= MESH_MAX_ROWS) return 0;
    return nx * ny * nz * 3;
}

#define MESH_CHECK_LATTICE(name)                                                                                                              \
    PAG_CHECK_ARG(mesh_rows(nx, ny, nz) > 0, name ": lattice %lld x %lld x %lld: every axis needs 2 points, fewer than 2^31 cells and 2^32 / 3 points", \
                  (long long)nx, (long long)ny, (long long)nz)

}  // namespace

extern "C" int64_t pag_mesh_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    const int64_t rows = mesh_rows(nx, ny, nz);
    if (rows == 0) return 0;
    const int64_t nb = oa_blocks(rows);
    return oa_align(nb * 8) + oa_align(nb * 4);
}

extern "C" int pag_mesh_vertices(const float *field, int64_t nx, int64_t ny, int64_t nz, float iso, const float *lo_host, float h,
                                 const int32_t *index0_host, float *vertices, float *normals, int64_t cap, int32_t *cell_vertex, int64_t *count,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    MESH_CHECK_LATTICE("pag_mesh_vertices");
    PAG_CHECK_ARG(cap >= 0 && lo_host && index0_host, "pag_mesh_vertices: cap %lld < 0 or NULL lo_host / index0_host", (long long)cap);
    PAG_CHECK_ARG(field && cell_vertex && count && (cap == 0 || (vertices && normals)), "pag_mesh_vertices: NULL field / cell_vertex / counter / output");
    for (int x = 0; x < 3; ++x)
        PAG_CHECK_ARG(index0_host[x] >= 0 && (int64_t)index0_host[x] + (x == 0 ? nx : (x == 1 ? ny : nz)) < MESH_MAX_CELLS,
                      "pag_mesh_vertices: index0[%d] = %d: a global index leaves [0, 2^31)", x, index0_host[x]);
    MeshCellPred p = {};
    p.n = (nx - 1) * (ny - 1) * (nz - 1);
    p.field = field, p.cy = (uint32_t)(ny - 1), p.cz = (uint32_t)(nz - 1), p.sx = ny * nz, p.sy = nz, p.iso = iso;
    MeshVertexWrite w = {};
    for (int x = 0; x < 3; ++x) w.lo[x] = lo_host[x], w.index0[x] = index0_host[x];
    w.h = h, w.vertices = vertices, w.normals = normals, w.cell_vertex = cell_vertex, w.cap = cap;
    hipStream_t st = (hipStream_t)stream;
    return oa_append("pag_mesh_vertices", "pag_mesh_workspace_bytes(nx, ny, nz)", pag_mesh_workspace_bytes(nx, ny, nz), p, count, workspace,
                     workspace_bytes, st, [&](dim3 grid, dim3 block, const int64_t *block_offset) {
                         hipLaunchKernelGGL(mesh_vertex_write_kernel, grid, block, 0, st, p, w, block_offset);
                     });
}

extern "C" int pag_mesh_faces(const float *field, int64_t nx, int64_t ny, int64_t nz, float iso, const int32_t *cell_vertex, int32_t *faces,
                              int64_t cap, int64_t *count, void *workspace, int64_t workspace_bytes, void *stream) {
    MESH_CHECK_LATTICE("pag_mesh_faces");
    PAG_CHECK_ARG(cap >= 0 && field && cell_vertex && count && (cap == 0 || faces), "pag_mesh_faces: cap %lld < 0 or NULL field / cell_vertex / counter / output",
                  (long long)cap);
    MeshEdgePred p = {};
    p.n = mesh_rows(nx, ny, nz);
    p.field = field, p.cell_vertex = cell_vertex, p.nx = (uint32_t)nx, p.ny = (uint32_t)ny, p.nz = (uint32_t)nz, p.iso = iso;
    hipStream_t st = (hipStream_t)stream;
    return oa_append("pag_mesh_faces", "pag_mesh_workspace_bytes(nx, ny, nz)", pag_mesh_workspace_bytes(nx, ny, nz), p, count, workspace, workspace_bytes,
                     st, [&](dim3 grid, dim3 block, const int64_t *block_offset) {
                         hipLaunchKernelGGL(mesh_face_write_kernel, grid, block, 0, st, p, faces, cap, block_offset);
                     });
}
