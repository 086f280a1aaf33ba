// mesh_test.cpp — stand-alone CPU checks of mesh.cpp (no HIP, no Python), run plain and under the address
// and undefined-behaviour sanitizers by tests/test_mesh_cpu.py, all on exactly sized heap arrays.
//   mesh_test [DIR]        the descriptor check field by field, the hand cases of the rule (one inside point,
//                          a NaN end, the empty and the all-inside lattice), an analytic sphere's closed
//                          surface, the count-then-fill form; with DIR, both encoders write there
//   mesh_test run IN OUT   rmr_surface_nets on a volume file: IN = rmr_volume_desc, iso, the distances;
//                          OUT = n_vertices, n_quads (uint64), the vertices, the quads
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rmr_mesh_rule.h"

namespace {
int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

rmr_volume_desc lattice(float ox, float oy, float oz, float spacing, int nx, int ny, int nz) {
    rmr_volume_desc d;
    d.origin[0] = ox; d.origin[1] = oy; d.origin[2] = oz;
    d.spacing = spacing;
    d.n[0] = nx; d.n[1] = ny; d.n[2] = nz;
    return d;
}

struct Mesh {
    int rc = 0;
    rmr_mesh_info info{};
    std::vector<float> v;
    std::vector<uint32_t> q;
};
// count, then fill into exactly sized arrays
Mesh extract(const std::vector<float>& dist, const rmr_volume_desc& d, float iso) {
    Mesh m;
    m.rc = rmr_surface_nets(dist.data(), &d, iso, nullptr, 0, nullptr, 0, &m.info);
    if (m.rc != RMR_OK) return m;
    m.v.resize(3 * (size_t)m.info.n_vertices);
    m.q.resize(4 * (size_t)m.info.n_quads);
    float dummy_v = 0.0f;
    uint32_t dummy_q = 0;
    rmr_mesh_info again{};
    m.rc = rmr_surface_nets(dist.data(), &d, iso, m.v.empty() ? &dummy_v : m.v.data(), m.v.size() / 3,
                            m.q.empty() ? &dummy_q : m.q.data(), m.q.size() / 4, &again);
    CHECK(again.n_vertices == m.info.n_vertices && again.n_quads == m.info.n_quads);
    return m;
}

std::vector<float> sphere_volume(const rmr_volume_desc& d, float r) {
    std::vector<float> dist((size_t)d.n[0] * d.n[1] * d.n[2]);
    size_t k = 0;
    for (int iz = 0; iz < d.n[2]; iz++)
        for (int iy = 0; iy < d.n[1]; iy++)
            for (int ix = 0; ix < d.n[0]; ix++) {
                const double x = rmr::lattice_coord(d.origin[0], ix, d.spacing), y = rmr::lattice_coord(d.origin[1], iy, d.spacing),
                             z = rmr::lattice_coord(d.origin[2], iz, d.spacing);
                dist[k++] = (float)(std::sqrt(x * x + y * y + z * z) - (double)r);
            }
    return dist;
}

void check_descriptor() {
    const char* bad = "?";
    rmr_volume_desc d = lattice(0, 0, 0, 0.5f, 2, 2, 2);
    CHECK(rmr_check_volume(&d, &bad) == RMR_OK && bad == nullptr);
    CHECK(rmr_check_volume(&d, nullptr) == RMR_OK);
    CHECK(rmr_check_volume(nullptr, &bad) == RMR_E_INVALID && std::string(bad) == "desc");
    auto field = [&](rmr_volume_desc e) {
        const char* b = nullptr;
        return rmr_check_volume(&e, &b) == RMR_E_INVALID && b ? std::string(b) : std::string("ok");
    };
    rmr_volume_desc e = d;
    e.origin[1] = kNaN; CHECK(field(e) == "origin");
    e = d; e.origin[2] = -kInf; CHECK(field(e) == "origin");
    e = d; e.spacing = 0.0f; CHECK(field(e) == "spacing");
    e = d; e.spacing = -1.0f; CHECK(field(e) == "spacing");
    e = d; e.spacing = kInf; CHECK(field(e) == "spacing");
    e = d; e.spacing = kNaN; CHECK(field(e) == "spacing");
    e = d; e.n[0] = 1; CHECK(field(e) == "n");
    e = d; e.n[2] = 4097; CHECK(field(e) == "n");
    e = d; e.n[1] = -5; CHECK(field(e) == "n");
    e = d; e.n[0] = 4096; e.n[1] = 4096; e.n[2] = 65; CHECK(field(e) == "points");
    e.n[2] = 64; CHECK(field(e) == "ok");
}

void check_hand_cases() {
    // one inside point in the middle of a 3^3 lattice: 8 active cells, 6 quads (one per edge at the point), and
    // crossings at t = 0.25 from the inside point (d = -1 against +3)
    rmr_volume_desc d = lattice(-1.0f, -1.0f, -1.0f, 1.0f, 3, 3, 3);
    std::vector<float> dist(27, 3.0f);
    dist[13] = -1.0f;
    Mesh m = extract(dist, d, 0.0f);
    CHECK(m.rc == RMR_OK && m.info.n_vertices == 8 && m.info.n_quads == 6);
    // vertex 0 is cell (0,0,0): its inside corner is corner 7; crossing edges: x at (1,1), y at (1,1), z at (1,1),
    // each 0.75 along its own axis and 1 on the others: mean (2.75 / 3) per axis
    const float want = -1.0f + 1.0f * ((((0.75f + 1.0f) + 1.0f)) / 3.0f);
    CHECK(m.v.size() == 24 && m.v[0] == want && m.v[1] == want && m.v[2] == want);
    // the first quad: the edge from point 4 = (1, 1, 0) along z, lower end outside: reversed order of the
    // cells (0,0,0) (1,0,0) (1,1,0) (0,1,0) = vertices 0 1 3 2
    CHECK(m.q.size() == 24 && m.q[0] == 2 && m.q[1] == 3 && m.q[2] == 1 && m.q[3] == 0);
    // a NaN or infinite end: the crossing is 0.5; a NaN point is outside
    CHECK(rmr::mesh_crossing(-1.0f, kNaN, 0.0f) == 0.5f && rmr::mesh_crossing(-kInf, kInf, 0.0f) == 0.5f);
    CHECK(rmr::mesh_crossing(-1.0f, kInf, 0.0f) == 0.0f && rmr::mesh_crossing(-1.0f, 3.0f, 0.0f) == 0.25f);
    CHECK(!rmr::mesh_inside(kNaN, 0.0f) && !rmr::mesh_inside(0.0f, 0.0f) && rmr::mesh_inside(-0.0f, 1e-30f));
    std::fill(dist.begin(), dist.end(), kNaN);
    dist[13] = -1.0f;
    m = extract(dist, d, 0.0f);
    CHECK(m.rc == RMR_OK && m.info.n_vertices == 8 && m.info.n_quads == 6);
    for (float x : m.v) CHECK(x == x && std::fabs(x) <= 1.0f);
    // nothing inside, everything inside
    std::fill(dist.begin(), dist.end(), 2.0f);
    m = extract(dist, d, 0.0f);
    CHECK(m.rc == RMR_OK && m.info.n_vertices == 0 && m.info.n_quads == 0);
    m = extract(dist, d, 2.5f);
    CHECK(m.rc == RMR_OK && m.info.n_vertices == 0 && m.info.n_quads == 0);
    // argument checks; a fill into arrays that are too small writes nothing
    rmr_mesh_info info{};
    CHECK(rmr_surface_nets(nullptr, &d, 0.0f, nullptr, 0, nullptr, 0, &info) == RMR_E_INVALID);
    CHECK(rmr_surface_nets(dist.data(), &d, kNaN, nullptr, 0, nullptr, 0, &info) == RMR_E_INVALID);
    CHECK(rmr_surface_nets(dist.data(), &d, 0.0f, nullptr, 0, nullptr, 0, nullptr) == RMR_E_INVALID);
    dist[13] = -1.0f;
    std::vector<float> v(3 * 7, 9.0f);
    std::vector<uint32_t> q(4 * 6, 9u);
    CHECK(rmr_surface_nets(dist.data(), &d, 0.0f, v.data(), 7, q.data(), 6, &info) == RMR_E_INVALID);
    CHECK(info.n_vertices == 8 && info.n_quads == 6 && v[0] == 9.0f && q[0] == 9u);
}

// the unit sphere in a 17^3 lattice: closed, oriented outward, Euler number 2, vertices near the sphere
void check_sphere() {
    const rmr_volume_desc d = lattice(-1.5f, -1.5f, -1.5f, 3.0f / 16.0f, 17, 17, 17);
    const Mesh m = extract(sphere_volume(d, 1.0f), d, 0.0f);
    CHECK(m.rc == RMR_OK && m.info.n_vertices > 100 && m.info.n_quads > 100);
    std::map<std::pair<uint32_t, uint32_t>, int> directed;
    for (size_t i = 0; i < m.q.size(); i += 4)
        for (int j = 0; j < 4; j++) {
            CHECK(m.q[i + j] < m.info.n_vertices);
            directed[{m.q[i + j], m.q[i + (j + 1) % 4]}]++;
        }
    size_t edges = 0;
    for (const auto& e : directed) {
        CHECK(e.second == 1);
        CHECK(directed.count({e.first.second, e.first.first}) == 1);
        edges++;
    }
    CHECK(edges % 2 == 0);
    CHECK((long long)m.info.n_vertices - (long long)(edges / 2) + (long long)m.info.n_quads == 2);
    double volume = 0.0, worst = 0.0;
    for (size_t i = 0; i < m.q.size(); i += 4) {
        const uint32_t tri[2][3] = {{m.q[i], m.q[i + 1], m.q[i + 2]}, {m.q[i], m.q[i + 2], m.q[i + 3]}};
        for (const auto& t : tri) {
            const float *a = &m.v[3 * t[0]], *b = &m.v[3 * t[1]], *c = &m.v[3 * t[2]];
            volume += ((double)a[0] * ((double)b[1] * c[2] - (double)b[2] * c[1]) - (double)a[1] * ((double)b[0] * c[2] - (double)b[2] * c[0]) +
                       (double)a[2] * ((double)b[0] * c[1] - (double)b[1] * c[0])) / 6.0;
        }
    }
    for (size_t i = 0; i < m.v.size(); i += 3)
        worst = std::fmax(worst, std::fabs(std::sqrt((double)m.v[i] * m.v[i] + (double)m.v[i + 1] * m.v[i + 1] + (double)m.v[i + 2] * m.v[i + 2]) - 1.0));
    std::printf("sphere: %llu vertices, %llu quads, volume %.4f, worst |r - 1| %.4f\n", (unsigned long long)m.info.n_vertices,
                (unsigned long long)m.info.n_quads, volume, worst);
    CHECK(volume > 3.8 && volume < 4.4);   // 4 pi / 3 = 4.19
    CHECK(worst < 0.5 * 3.0 / 16.0);
}

void check_encoders(const std::string& dir) {
    const rmr_volume_desc d = lattice(-1.0f, -1.0f, -1.0f, 1.0f, 3, 3, 3);
    std::vector<float> dist(27, 3.0f);
    dist[13] = -1.0f;
    const Mesh m = extract(dist, d, 0.0f);
    std::vector<float> nrm(m.v), ids(8, 2.0f);
    CHECK(rmr_encode_obj((dir + "/a.obj").c_str(), m.v.data(), nrm.data(), 8, m.q.data(), 6) == RMR_OK);
    CHECK(rmr_encode_obj((dir + "/b.obj").c_str(), m.v.data(), nullptr, 8, m.q.data(), 6) == RMR_OK);
    CHECK(rmr_encode_ply((dir + "/a.ply").c_str(), m.v.data(), nrm.data(), ids.data(), 8, m.q.data(), 6) == RMR_OK);
    CHECK(rmr_encode_ply((dir + "/b.ply").c_str(), m.v.data(), nullptr, nullptr, 8, m.q.data(), 6) == RMR_OK);
    CHECK(rmr_encode_obj((dir + "/empty.obj").c_str(), nullptr, nullptr, 0, nullptr, 0) == RMR_OK);
    CHECK(rmr_encode_obj((dir + "/no/such/dir.obj").c_str(), m.v.data(), nullptr, 8, m.q.data(), 6) == RMR_E_IO);
    CHECK(rmr_encode_ply((dir + "/c.ply").c_str(), m.v.data(), nullptr, nullptr, 7, m.q.data(), 6) == RMR_E_INVALID);   // index 7
    CHECK(rmr_encode_obj(nullptr, m.v.data(), nullptr, 8, m.q.data(), 6) == RMR_E_INVALID);
}

int run_file(const char* in_path, const char* out_path) {
    std::FILE* f = std::fopen(in_path, "rb");
    if (!f) return 3;
    rmr_volume_desc d;
    float iso = 0.0f;
    bool ok = std::fread(&d, sizeof d, 1, f) == 1 && std::fread(&iso, sizeof iso, 1, f) == 1 && rmr_check_volume(&d, nullptr) == RMR_OK;
    std::vector<float> dist;
    if (ok) {
        dist.resize((size_t)d.n[0] * d.n[1] * d.n[2]);
        ok = std::fread(dist.data(), sizeof(float), dist.size(), f) == dist.size();
    }
    std::fclose(f);
    if (!ok) return 3;
    const Mesh m = extract(dist, d, iso);
    if (m.rc != RMR_OK || failures) return 4;
    f = std::fopen(out_path, "wb");
    if (!f) return 3;
    const uint64_t head[2] = {m.info.n_vertices, m.info.n_quads};
    std::fwrite(head, sizeof head, 1, f);
    if (!m.v.empty()) std::fwrite(m.v.data(), sizeof(float), m.v.size(), f);
    if (!m.q.empty()) std::fwrite(m.q.data(), sizeof(uint32_t), m.q.size(), f);
    if (std::fclose(f) != 0) return 3;
    std::printf("mesh_test run ok: %llu vertices, %llu quads\n", (unsigned long long)head[0], (unsigned long long)head[1]);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    static_assert(sizeof(rmr_volume_desc) == 28, "rmr_volume_desc is 28 bytes");
    if (argc == 4 && std::string(argv[1]) == "run") return run_file(argv[2], argv[3]);
    check_descriptor();
    check_hand_cases();
    check_sphere();
    if (argc == 2) check_encoders(argv[1]);
    if (failures) {
        std::printf("mesh_test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("mesh_test ok\n");
    return 0;
}
