// LabelTransfer.cpp -- the flow of the reference's example/GetLabelUsingKDTree.cpp over the class surface: ScanNet's semantic labels, and through a
// second hop its instance labels, moved from the annotated mesh onto a reconstructed model by one exact nearest-neighbour query per vertex
// (kept when the SQUARED distance is below --max-dist, as the example compares `dists[0] < max_distance`).
//
//   LabelTransfer <model.ply> <annotated.ply> [--instances labels.i32 --highres mesh.ply] [--path host|device] [--max-dist 0.1] [--dump DIR] [--warmup 0] [--repeat 1]
//   LabelTransfer --synthetic N M SEED [--path host|device] [--max-dist 0.1] [--dump DIR] [--warmup 0] [--repeat 1]
//   LabelTransfer --cloud T.f32 [--labels L.i32 | --labels16 L.u16] [--default D] --batch Q.f32 [--batch ... | --cloud ...] [--path host|device] [--max-dist inf] --dump DIR
//
//   LabelTransfer --ply-write OUT.ply --cloud P.f32 [--normals N.f32] [--colors C.f32] [--faces F.u32] [--labels16 L.u16 | --labels L.i32] [--ascii]
//   LabelTransfer --ply-read IN.ply --dump DIR
//
//   annotated.ply   a mesh with a `ushort label` vertex property (ScanNet's *_vh_clean_2.labels.ply)
//   --instances     one little-endian int32 per vertex of --highres (what the example takes from ScanNet's JSON files through
//                   tool::ReadIntanceInfoFromScannet, which needs a JSON parser this surface does not carry); --highres is *_vh_clean.ply
//   --path host     OP_RUNTIME_OPT_NEAREST_BATCH 0: KDTree<>::NearestBatch is the loop of KnnSearch(q, ..., 1) the example writes; no device is touched
//   --path device   the option at 1: the same calls forward to op_nn_index_query
//   --synthetic     N model vertices, M annotated vertices (and 2 M high-resolution ones) planted on the walls of a room, without any input file
//   --warmup W      whole untimed passes (index build, the three query batches, the gathers) before the timed ones: first launches load code objects
//   --repeat K      timed passes; the stage times printed are medians over them, total_ms_runs lists every pass
//   --cloud/--batch raw little-endian n x 3 float32 files, in argument order: --cloud builds the tree (BuildTree), every --batch runs NearestBatch on it
//                   (and tool::TransferLabels when labels were given) and dumps batch_K_idx.i32, batch_K_dist.f32, batch_K_labels.i32 / .u16
//   --ply-write     tool::WritePLY of raw arrays with a `label` vertex property (ushort or int) and one comment line
//   --ply-read      tool::ReadPLY asking for `label` -> points.f32 normals.f32 colors.f32 faces.u32 labels.bin and result.json (the label type and count);
//                   and TriangleMesh::LoadFromPLY of the same file -> mesh_points.f32 mesh_normals.f32 mesh_colors.f32 mesh_faces.u32
//   --dump DIR      semantic_idx.i32 semantic_labels.u16 hop1_idx.i32 hop1_labels.i32 hop2_idx.i32 instance_labels.i32, the inputs of a synthetic
//                   run (model_points.f32 annotated_points.f32 annotated_labels.u16 highres_points.f32 highres_labels.i32) and result.json
// Writes Labeled_model.ply (into DIR when given, else the working directory) with the `label` property; prints one JSON line with the time of
// every stage (read, index build, query, gather, write) and the tied / doubtful counts of the device path.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Geometry/KDTree.h"
#include "Geometry/TriangleMesh.h"
#include "Tool/PLYManager.h"
#include "onepiece_hip.h"
using namespace one_piece;

namespace {

double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class V>
bool WriteRaw(const std::string& file, const V* data, size_t count) {
    std::ofstream os(file.c_str(), std::ios::binary);
    if (count) os.write(reinterpret_cast<const char*>(data), static_cast<std::streamsize>(count * sizeof(V)));
    return static_cast<bool>(os);
}
bool WritePoints(const std::string& file, const geometry::Point3List& p) { return WriteRaw(file, p.empty() ? nullptr : p[0].data(), p.size() * 3); }
template <class V>
bool ReadRaw(const std::string& file, std::vector<V>& out) {
    std::ifstream is(file.c_str(), std::ios::binary | std::ios::ate);
    if (!is) return false;
    const std::streamsize bytes = is.tellg();
    if (bytes < 0 || bytes % static_cast<std::streamsize>(sizeof(V)) != 0) return false;
    out.assign(static_cast<size_t>(bytes) / sizeof(V), V());
    is.seekg(0);
    return bytes == 0 || static_cast<bool>(is.read(reinterpret_cast<char*>(out.data()), bytes));
}
bool ReadPoints(const std::string& file, geometry::Point3List& out) {
    std::vector<float> raw;
    if (!ReadRaw(file, raw) || raw.size() % 3 != 0) return false;
    out.resize(raw.size() / 3);
    for (size_t i = 0; i < out.size(); ++i) out[i] = geometry::Point3(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]);
    return true;
}

struct Rng { // a 64-bit LCG: the same clouds on every platform
    uint64_t s;
    double Next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<double>(s >> 11) * (1.0 / 9007199254740992.0); }
};
// a point on the walls, floor and ceiling of a 6 x 3 x 5 m room, and the label of the patch it lies in
geometry::Point3 WallPoint(Rng& r, int& patch) {
    const float half[3] = {3.0f, 1.5f, 2.5f};
    const int face = static_cast<int>(r.Next() * 6) % 6, axis = face / 2;
    float p[3];
    for (int k = 0; k < 3; ++k) p[k] = static_cast<float>((2 * r.Next() - 1) * half[k]);
    p[axis] = (face & 1) ? half[axis] : -half[axis];
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    patch = face * 16 + (static_cast<int>((p[u] + half[u]) / (2 * half[u]) * 3.999f) * 4 + static_cast<int>((p[v] + half[v]) / (2 * half[v]) * 3.999f));
    return geometry::Point3(p[0], p[1], p[2]);
}

int RawMode(const std::vector<std::pair<std::string, std::string> >& steps, const std::string& labels_file, const std::string& labels16_file, int default_label,
            float max_sq, const std::string& dump, const std::string& path) {
    geometry::KDTree<> tree;
    geometry::Point3List targets;
    std::vector<int> labels;
    std::vector<unsigned short> labels16;
    if (!labels_file.empty() && !ReadRaw(labels_file, labels)) { std::cout << "cannot read " << labels_file << std::endl; return 3; }
    if (!labels16_file.empty() && !ReadRaw(labels16_file, labels16)) { std::cout << "cannot read " << labels16_file << std::endl; return 3; }
    int batch = 0;
    std::ostringstream js;
    js << "{\"path\": \"" << path << "\", \"batches\": [";
    for (size_t s = 0; s < steps.size(); ++s) {
        if (steps[s].first == "cloud") {
            if (!ReadPoints(steps[s].second, targets)) { std::cout << "cannot read " << steps[s].second << std::endl; return 3; }
            tree.BuildTree(targets);
            continue;
        }
        geometry::Point3List queries;
        if (!ReadPoints(steps[s].second, queries)) { std::cout << "cannot read " << steps[s].second << std::endl; return 3; }
        std::vector<int> idx;
        std::vector<float> dist;
        tree.NearestBatch(queries, idx, dist, max_sq);
        std::ostringstream name;
        name << dump << "/batch_" << batch;
        const std::string tag = name.str();
        bool ok = WriteRaw(tag + "_idx.i32", idx.data(), idx.size()) && WriteRaw(tag + "_dist.f32", dist.data(), dist.size());
        if (!labels.empty() || (!labels_file.empty() && targets.empty())) {
            std::vector<int> out;
            tool::TransferLabels(targets, labels, queries, max_sq, default_label, out);
            ok = ok && WriteRaw(tag + "_labels.i32", out.data(), out.size());
        }
        if (!labels16.empty()) {
            std::vector<unsigned short> out;
            tool::TransferLabels(targets, labels16, queries, max_sq, static_cast<unsigned short>(default_label), out);
            ok = ok && WriteRaw(tag + "_labels.u16", out.data(), out.size());
        }
        if (!ok) { std::cout << "cannot write to " << dump << std::endl; return 3; }
        unsigned long long q = 0, t = 0, d = 0;
        tree.NearestBatchStats(q, t, d);
        js << (batch ? ", " : "") << "{\"queries\": " << queries.size() << ", \"index_queries\": " << q << ", \"tied\": " << t << ", \"doubtful\": " << d << "}";
        ++batch;
    }
    js << "]}";
    std::cout << js.str() << std::endl;
    std::ofstream os((dump + "/result.json").c_str());
    os << js.str() << std::endl;
    return 0;
}

double Median(std::vector<double> v) {
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

bool WriteFaces(const std::string& file, const geometry::Point3uiList& f) { return WriteRaw(file, f.empty() ? nullptr : f[0].data(), f.size() * 3); }

int PlyWrite(const std::string& out, const std::string& cloud, const std::string& normals, const std::string& colors, const std::string& faces, const std::string& labels_file,
             const std::string& labels16_file, bool ascii) {
    geometry::Point3List p, n, c;
    geometry::Point3uiList tri;
    std::vector<unsigned> raw_faces;
    std::vector<int> labels;
    std::vector<unsigned short> labels16;
    if (!ReadPoints(cloud, p) || (!normals.empty() && !ReadPoints(normals, n)) || (!colors.empty() && !ReadPoints(colors, c)) || (!faces.empty() && !ReadRaw(faces, raw_faces)) ||
        (!labels_file.empty() && !ReadRaw(labels_file, labels)) || (!labels16_file.empty() && !ReadRaw(labels16_file, labels16))) {
        std::cout << "cannot read the arrays" << std::endl;
        return 3;
    }
    for (size_t i = 0; i + 2 < raw_faces.size(); i += 3) tri.push_back(geometry::Point3ui(raw_faces[i], raw_faces[i + 1], raw_faces[i + 2]));
    std::vector<tool::AdditionalElement> extra;
    if (!labels_file.empty() || !labels16_file.empty()) {
        tool::AdditionalElement e;
        e.element_key = "vertex";
        e.element_property.push_back("label");
        const bool wide = !labels_file.empty();
        e.type = wide ? tinyply::Type::INT32 : tinyply::Type::UINT16;
        e.count = wide ? labels.size() : labels16.size();
        e.byte_size = e.count * (wide ? 4 : 2);
        e.data = wide ? reinterpret_cast<unsigned char*>(labels.data()) : reinterpret_cast<unsigned char*>(labels16.data());
        extra.push_back(e);
    }
    return tool::WritePLY(out, p, n, c, tri, std::vector<std::string>(1, "each vertex will have semantic labels."), extra, ascii) ? 0 : 3;
}

int PlyRead(const std::string& in, const std::string& dump) {
    geometry::Point3List p, n, c;
    geometry::Point3uiList tri;
    std::vector<tool::AdditionalElement> extra(1);
    extra[0].element_key = "vertex";
    extra[0].element_property.push_back("label");
    if (!tool::ReadPLY(in, p, n, c, tri, extra)) return 3;
    bool ok = WritePoints(dump + "/points.f32", p) && WritePoints(dump + "/normals.f32", n) && WritePoints(dump + "/colors.f32", c) && WriteFaces(dump + "/faces.u32", tri) &&
              WriteRaw(dump + "/labels.bin", extra[0].data, extra[0].byte_size);
    geometry::TriangleMesh mesh;
    ok = ok && mesh.LoadFromPLY(in) && WritePoints(dump + "/mesh_points.f32", mesh.points) && WritePoints(dump + "/mesh_normals.f32", mesh.normals) &&
         WritePoints(dump + "/mesh_colors.f32", mesh.colors) && WriteFaces(dump + "/mesh_faces.u32", mesh.triangles);
    std::ostringstream js;
    js << "{\"vertices\": " << p.size() << ", \"faces\": " << tri.size() << ", \"label_type\": " << static_cast<int>(extra[0].type) << ", \"label_count\": " << extra[0].count
       << ", \"label_bytes\": " << extra[0].byte_size << "}";
    delete[] extra[0].data;
    if (!ok) { std::cout << "cannot read " << in << " or write to " << dump << std::endl; return 3; }
    std::cout << js.str() << std::endl;
    std::ofstream os((dump + "/result.json").c_str());
    os << js.str() << std::endl;
    return 0;
}

} // namespace

int main(int argc, char** argv) {
    std::string path = "host", dump, instances_file, highres_file, labels_file, labels16_file, ply_write, ply_read, normals_file, colors_file, faces_file;
    bool ascii = false;
    int warmup = 0, repeat = 1;
    std::vector<std::string> positional;
    std::vector<std::pair<std::string, std::string> > steps;
    float max_sq = 0.1f; // the example's max_distance, compared with the squared distance
    long synthetic[3] = {0, 0, 0};
    bool is_synthetic = false;
    int default_label = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--instances" && i + 1 < argc) instances_file = argv[++i];
        else if (a == "--highres" && i + 1 < argc) highres_file = argv[++i];
        else if (a == "--max-dist" && i + 1 < argc) max_sq = static_cast<float>(std::atof(argv[++i])); // "inf" = no cutoff
        else if (a == "--labels" && i + 1 < argc) labels_file = argv[++i];
        else if (a == "--labels16" && i + 1 < argc) labels16_file = argv[++i];
        else if (a == "--ply-write" && i + 1 < argc) ply_write = argv[++i];
        else if (a == "--ply-read" && i + 1 < argc) ply_read = argv[++i];
        else if (a == "--normals" && i + 1 < argc) normals_file = argv[++i];
        else if (a == "--colors" && i + 1 < argc) colors_file = argv[++i];
        else if (a == "--faces" && i + 1 < argc) faces_file = argv[++i];
        else if (a == "--ascii") ascii = true;
        else if (a == "--warmup" && i + 1 < argc) warmup = std::atoi(argv[++i]);
        else if (a == "--repeat" && i + 1 < argc) repeat = std::atoi(argv[++i]);
        else if (a == "--default" && i + 1 < argc) default_label = std::atoi(argv[++i]);
        else if ((a == "--cloud" || a == "--batch") && i + 1 < argc) { steps.push_back(std::make_pair(a.substr(2), std::string(argv[i + 1]))); ++i; }
        else if (a == "--synthetic" && i + 3 < argc) { is_synthetic = true; for (int k = 0; k < 3; ++k) synthetic[k] = std::atol(argv[++i]); }
        else if (a.compare(0, 2, "--") != 0) positional.push_back(a);
        else { std::cout << "unknown argument " << a << std::endl; return 2; }
    }
    if (!ply_write.empty() && steps.size() == 1 && steps[0].first == "cloud")
        return PlyWrite(ply_write, steps[0].second, normals_file, colors_file, faces_file, labels_file, labels16_file, ascii);
    if (!ply_read.empty() && !dump.empty()) return PlyRead(ply_read, dump);
    const bool raw = !steps.empty();
    if ((path != "host" && path != "device") || (!raw && !is_synthetic && positional.size() != 2) || (raw && dump.empty()) || (instances_file.empty() != highres_file.empty()) ||
        (is_synthetic && (synthetic[0] < 0 || synthetic[1] < 0)) || warmup < 0 || repeat < 1) {
        std::cout << "Usage: LabelTransfer <model.ply> <annotated.ply> [--instances labels.i32 --highres mesh.ply] [--path host|device] [--max-dist 0.1] [--dump DIR]\n"
                     "       LabelTransfer --synthetic N M SEED [--path host|device] [--max-dist 0.1] [--dump DIR]\n"
                     "       LabelTransfer --cloud T.f32 [--labels L.i32 | --labels16 L.u16] [--default D] --batch Q.f32 ... --dump DIR [--path host|device] [--max-dist inf]\n"
                     "       LabelTransfer --ply-write OUT.ply --cloud P.f32 [--normals N.f32] [--colors C.f32] [--faces F.u32] [--labels16 L.u16 | --labels L.i32] [--ascii]\n"
                     "       LabelTransfer --ply-read IN.ply --dump DIR" << std::endl;
        return 2;
    }
    if (op_runtime_set_option(OP_RUNTIME_OPT_NEAREST_BATCH, path == "host" ? 0 : 1) != OP_OK) { std::cout << op_last_error() << std::endl; return 3; }
    if (raw) return RawMode(steps, labels_file, labels16_file, default_label, max_sq, dump, path);

    // ---- read (or plant) the model, the annotated mesh and, for the instance pass, the high-resolution mesh ----
    double t = Now();
    geometry::TriangleMesh mesh, reference_mesh, high_res_mesh;
    std::vector<unsigned short> reference_labels;
    std::vector<int> reference_instance_labels;
    bool instances = !instances_file.empty();
    if (is_synthetic) {
        Rng rng = {static_cast<uint64_t>(synthetic[2]) * 2654435761ull + 12345ull};
        int patch = 0;
        for (long i = 0; i < synthetic[1]; ++i) { reference_mesh.points.push_back(WallPoint(rng, patch)); reference_labels.push_back(static_cast<unsigned short>(1 + patch)); }
        for (long i = 0; i < 2 * synthetic[1]; ++i) { high_res_mesh.points.push_back(WallPoint(rng, patch)); reference_instance_labels.push_back(patch % 7 == 0 ? -1 : 1000 + patch); }
        for (long i = 0; i < synthetic[0]; ++i) { // the model: the same walls, reconstructed with some noise; every 16th vertex floats well away from them
            geometry::Point3 p = WallPoint(rng, patch);
            const float noise = i % 16 == 15 ? 0.6f : 0.02f;
            for (int k = 0; k < 3; ++k) p(k) = p(k) * (i % 16 == 15 ? 0.5f : 1.0f) + static_cast<float>((2 * rng.Next() - 1) * noise);
            mesh.points.push_back(p);
        }
        instances = true;
    } else {
        if (!mesh.LoadFromPLY(positional[0])) return 3;
        std::vector<tool::AdditionalElement> additional_labels(1);
        additional_labels[0].element_key = "vertex";
        additional_labels[0].element_property.push_back("label");
        if (!tool::ReadPLY(positional[1], reference_mesh.points, reference_mesh.normals, reference_mesh.colors, reference_mesh.triangles, additional_labels)) return 3;
        if (additional_labels[0].type != tinyply::Type::UINT16 || additional_labels[0].count != reference_mesh.points.size()) {
            std::cout << "Error occurs when reading labels." << std::endl;
            delete[] additional_labels[0].data;
            return 3;
        }
        reference_labels.resize(additional_labels[0].count);
        if (additional_labels[0].byte_size) std::memcpy(reference_labels.data(), additional_labels[0].data, additional_labels[0].byte_size);
        delete[] additional_labels[0].data;
        if (instances) {
            if (!high_res_mesh.LoadFromPLY(highres_file) || !ReadRaw(instances_file, reference_instance_labels) || reference_instance_labels.size() != high_res_mesh.points.size()) {
                std::cout << "cannot read the instance labels (one int32 per vertex of --highres)" << std::endl;
                return 3;
            }
        }
    }
    const double ms_read = Now() - t;
    std::vector<double> runs_build, runs_query, runs_gather;
    std::vector<int> semantic_idx, hop1_idx, hop2_idx;
    std::vector<float> dists;
    std::vector<unsigned short> labels;
    std::vector<int> low_res_labels, instance_labels;
    unsigned long long stats[2][3] = {{0, 0, 0}, {0, 0, 0}};
    for (int pass = 0; pass < warmup + repeat; ++pass) { // every pass builds its trees (and device indices) anew, as a run of the example does
        double ms_build = 0, ms_query = 0, ms_gather = 0;
        // ---- semantic pass (GetLabelUsingKDTree.cpp:45-67) ----
        t = Now();
        geometry::KDTree<> kdtree;
        kdtree.BuildTree(reference_mesh.points);
        ms_build += Now() - t; t = Now();
        kdtree.NearestBatch(mesh.points, semantic_idx, dists, max_sq);
        ms_query += Now() - t; t = Now();
        labels.assign(mesh.points.size(), 0); // default semantic label is 0, means unannotated
        for (size_t i = 0; i < labels.size(); ++i) if (semantic_idx[i] >= 0) labels[i] = reference_labels[static_cast<size_t>(semantic_idx[i])];
        ms_gather += Now() - t;

        // ---- instance pass (:84-139): high-resolution mesh -> annotated mesh -> model; the annotated mesh's tree (and its device index) is the one built above ----
        low_res_labels.assign(reference_mesh.points.size(), 0);
        instance_labels.assign(mesh.points.size(), -1);
        if (instances) {
            t = Now();
            geometry::KDTree<> high_res_tree;
            high_res_tree.BuildTree(high_res_mesh.points);
            ms_build += Now() - t; t = Now();
            high_res_tree.NearestBatch(reference_mesh.points, hop1_idx, dists, max_sq);
            ms_query += Now() - t; t = Now();
            for (size_t i = 0; i < low_res_labels.size(); ++i) if (hop1_idx[i] >= 0) low_res_labels[i] = reference_instance_labels[static_cast<size_t>(hop1_idx[i])];
            ms_gather += Now() - t; t = Now();
            kdtree.NearestBatch(mesh.points, hop2_idx, dists, max_sq);
            ms_query += Now() - t; t = Now();
            for (size_t i = 0; i < instance_labels.size(); ++i) if (hop2_idx[i] >= 0) instance_labels[i] = low_res_labels[static_cast<size_t>(hop2_idx[i])];
            ms_gather += Now() - t;
            high_res_tree.NearestBatchStats(stats[1][0], stats[1][1], stats[1][2]);
        }
        kdtree.NearestBatchStats(stats[0][0], stats[0][1], stats[0][2]);
        if (pass >= warmup) { runs_build.push_back(ms_build); runs_query.push_back(ms_query); runs_gather.push_back(ms_gather); }
    }
    std::vector<double> runs_total;
    for (size_t k = 0; k < runs_build.size(); ++k) runs_total.push_back(runs_build[k] + runs_query[k] + runs_gather[k]);
    const double ms_build = Median(runs_build), ms_query = Median(runs_query), ms_gather = Median(runs_gather);

    // ---- write (:68-75) ----
    t = Now();
    std::vector<tool::AdditionalElement> out_labels(1);
    out_labels[0].element_key = "vertex";
    out_labels[0].element_property.push_back("label");
    out_labels[0].type = tinyply::Type::UINT16;
    out_labels[0].count = labels.size();
    out_labels[0].byte_size = labels.size() * sizeof(unsigned short);
    out_labels[0].data = reinterpret_cast<unsigned char*>(labels.data());
    std::vector<std::string> comments(1, "each vertex will have semantic labels.");
    const std::string out_ply = (dump.empty() ? std::string(".") : dump) + "/Labeled_model.ply";
    if (!tool::WritePLY(out_ply, mesh.points, mesh.normals, mesh.colors, mesh.triangles, comments, out_labels)) return 3;
    const double ms_write = Now() - t;

    if (!dump.empty()) {
        bool ok = WriteRaw(dump + "/semantic_idx.i32", semantic_idx.data(), semantic_idx.size()) && WriteRaw(dump + "/semantic_labels.u16", labels.data(), labels.size());
        if (instances)
            ok = ok && WriteRaw(dump + "/hop1_idx.i32", hop1_idx.data(), hop1_idx.size()) && WriteRaw(dump + "/hop1_labels.i32", low_res_labels.data(), low_res_labels.size()) &&
                 WriteRaw(dump + "/hop2_idx.i32", hop2_idx.data(), hop2_idx.size()) && WriteRaw(dump + "/instance_labels.i32", instance_labels.data(), instance_labels.size());
        if (is_synthetic)
            ok = ok && WritePoints(dump + "/model_points.f32", mesh.points) && WritePoints(dump + "/annotated_points.f32", reference_mesh.points) &&
                 WriteRaw(dump + "/annotated_labels.u16", reference_labels.data(), reference_labels.size()) && WritePoints(dump + "/highres_points.f32", high_res_mesh.points) &&
                 WriteRaw(dump + "/highres_labels.i32", reference_instance_labels.data(), reference_instance_labels.size());
        if (!ok) { std::cout << "cannot write to " << dump << std::endl; return 3; }
    }
    size_t labelled = 0, with_instance = 0;
    for (size_t i = 0; i < labels.size(); ++i) { labelled += labels[i] != 0; with_instance += instance_labels[i] >= 0; }
    std::ostringstream js;
    js << "{\"path\": \"" << path << "\", \"model\": " << mesh.points.size() << ", \"annotated\": " << reference_mesh.points.size() << ", \"highres\": " << high_res_mesh.points.size()
       << ", \"max_sq_dist\": " << max_sq << ", \"labelled\": " << labelled << ", \"with_instance\": " << with_instance
       << ", \"annotated_index\": {\"queries\": " << stats[0][0] << ", \"tied\": " << stats[0][1] << ", \"doubtful\": " << stats[0][2] << "}"
       << ", \"highres_index\": {\"queries\": " << stats[1][0] << ", \"tied\": " << stats[1][1] << ", \"doubtful\": " << stats[1][2] << "}"
       << ", \"ms\": {\"read\": " << ms_read << ", \"index_build\": " << ms_build << ", \"query\": " << ms_query << ", \"gather\": " << ms_gather << ", \"write\": " << ms_write
       << ", \"total\": " << Median(runs_total) << "}, \"warmup\": " << warmup << ", \"repeat\": " << repeat << ", \"total_ms_runs\": [";
    for (size_t k = 0; k < runs_total.size(); ++k) js << (k ? ", " : "") << runs_total[k];
    js << "]}";
    std::cout << js.str() << std::endl;
    if (!dump.empty()) { std::ofstream os((dump + "/result.json").c_str()); os << js.str() << std::endl; }
    return 0;
}
