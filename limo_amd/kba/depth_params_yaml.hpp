// depth_params_yaml.hpp — reader of mono_lidar_fusion_parameters.yaml into a limo_depth_params (include/limo_hip.h).
//
// The reference application hands the depth estimator this file as it is.  Its form is flat: an optional `%YAML:1.0` first
// line, then `key: value  # comment` lines; no nesting, no lists, no quoting - so the reader needs no YAML library.  Keys are
// the file's own spellings (pixelarea_search_witdh, histogram_segmentation_bin_witdh).  An unknown key or a value that does
// not parse is an error that names the line; keys absent from the file keep the value `out` holds (the caller fills it with
// limo_depth_default_params first).  ransac_seed and neighbors_count_min (the minimum count of the rectangle search; the
// file has one for the radius search only) are not keys of the file.  Header only, and it calls nothing of the C-ABI.
// The same reader in Python: limo_amd/depth_params.py.
#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "../../include/limo_hip.h"

namespace keyframe_bundle_adjustment {
namespace depth_params_yaml {

struct Key {
    const char* name;  // as spelled in the file
    size_t offset;
    bool is_double;
};

#define LIMO_DEPTH_KEY_I(field) {#field, offsetof(limo_depth_params, field), false}
#define LIMO_DEPTH_KEY_D(field) {#field, offsetof(limo_depth_params, field), true}
inline const Key* keys(size_t* n) {
    static const Key table[] = {
        LIMO_DEPTH_KEY_I(neighbor_search_mode),
        {"pixelarea_search_witdh", offsetof(limo_depth_params, pixelarea_search_width), false},
        LIMO_DEPTH_KEY_I(pixelarea_search_height),
        LIMO_DEPTH_KEY_I(pixelarea_search_offset_x),
        LIMO_DEPTH_KEY_I(pixelarea_search_offset_y),
        LIMO_DEPTH_KEY_I(do_use_nearestNeighborSearch),
        LIMO_DEPTH_KEY_I(nnSearch_count),
        LIMO_DEPTH_KEY_I(do_use_radiusSearch),
        LIMO_DEPTH_KEY_D(radiusSearch_radius),
        LIMO_DEPTH_KEY_I(radiusSearch_count_min),
        LIMO_DEPTH_KEY_I(do_use_histogram_segmentation),
        {"histogram_segmentation_bin_witdh", offsetof(limo_depth_params, histogram_segmentation_bin_width), true},
        LIMO_DEPTH_KEY_I(histogram_segmentation_min_pointcount),
        LIMO_DEPTH_KEY_I(do_use_depth_segmentation),
        LIMO_DEPTH_KEY_D(depth_segmentation_max_treshold_gradient),
        LIMO_DEPTH_KEY_D(depth_segmentation_max_neighbor_distance),
        LIMO_DEPTH_KEY_D(depth_segmentation_max_neighbor_distance_gradient),
        LIMO_DEPTH_KEY_D(depth_segmentation_max_seedpoint_to_seedpoint_distance),
        LIMO_DEPTH_KEY_D(depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient),
        LIMO_DEPTH_KEY_D(depth_segmentation_max_neighbor_to_seedpoint_distance),
        LIMO_DEPTH_KEY_D(depth_segmentation_max_neighbor_to_seedpoint_distance_gradient),
        LIMO_DEPTH_KEY_I(depth_segmentation_max_pointcount),
        LIMO_DEPTH_KEY_I(treshold_depth_enabled),
        LIMO_DEPTH_KEY_I(treshold_depth_mode),
        LIMO_DEPTH_KEY_D(treshold_depth_max),
        LIMO_DEPTH_KEY_D(treshold_depth_min),
        LIMO_DEPTH_KEY_I(treshold_depth_local_enabled),
        LIMO_DEPTH_KEY_I(treshold_depth_local_mode),
        LIMO_DEPTH_KEY_I(treshold_depth_local_valuetype),
        LIMO_DEPTH_KEY_D(treshold_depth_local_value),
        LIMO_DEPTH_KEY_I(do_use_PCA),
        LIMO_DEPTH_KEY_D(pca_debug),
        LIMO_DEPTH_KEY_D(pca_treshold_3_abs_min),
        LIMO_DEPTH_KEY_D(pca_treshold_3_2_rel_max),
        LIMO_DEPTH_KEY_D(pca_treshold_2_1_rel_min),
        LIMO_DEPTH_KEY_I(do_use_ransac_plane),
        LIMO_DEPTH_KEY_D(ransac_plane_distance_treshold),
        LIMO_DEPTH_KEY_D(ransac_plane_min_z),
        LIMO_DEPTH_KEY_D(ransac_plane_max_z),
        LIMO_DEPTH_KEY_I(ransac_plane_max_iterations),
        LIMO_DEPTH_KEY_D(ransac_plane_probability),
        LIMO_DEPTH_KEY_I(ransac_plane_use_refinement),
        LIMO_DEPTH_KEY_D(ransac_plane_refinement_treshold),
        LIMO_DEPTH_KEY_D(ransac_plane_point_distance_treshold),
        LIMO_DEPTH_KEY_I(ransac_plane_use_camx_treshold),
        LIMO_DEPTH_KEY_D(ransac_plane_treshold_camx),
        LIMO_DEPTH_KEY_I(plane_estimator_use_triangle_maximation),
        LIMO_DEPTH_KEY_I(plane_estimator_use_leastsquares),
        LIMO_DEPTH_KEY_I(plane_estimator_use_mestimator),
        LIMO_DEPTH_KEY_D(plane_estimator_z_x_min_relation),
        LIMO_DEPTH_KEY_I(do_use_cut_behind_camera),
        LIMO_DEPTH_KEY_I(do_use_triangle_size_maximation),
        LIMO_DEPTH_KEY_I(do_check_triangleplanar_condition),
        LIMO_DEPTH_KEY_D(triangleplanar_crossnorm_treshold),
        LIMO_DEPTH_KEY_D(viewray_plane_orthoganality_treshold),
        LIMO_DEPTH_KEY_I(do_debug_singleFeatures),
        LIMO_DEPTH_KEY_I(do_publish_points),
        LIMO_DEPTH_KEY_I(do_depth_calc_statistics),
    };
    *n = sizeof(table) / sizeof(table[0]);
    return table;
}
#undef LIMO_DEPTH_KEY_I
#undef LIMO_DEPTH_KEY_D

inline std::string trim(const std::string& s) {
    const size_t a = s.find_first_not_of(" \t\r\n");
    if (a == std::string::npos) return "";
    return s.substr(a, s.find_last_not_of(" \t\r\n") - a + 1);
}

// One line of the file into `out`.  Returns false and fills `err` (without the line number) when it cannot be read.
inline bool parseLine(const std::string& raw, limo_depth_params* out, std::string* err) {
    const std::string line = trim(raw.substr(0, raw.find('#')));
    if (line.empty()) return true;
    const size_t colon = line.find(':');
    const std::string key = trim(line.substr(0, colon)), value = colon == std::string::npos ? "" : trim(line.substr(colon + 1));
    size_t n = 0;
    const Key* table = keys(&n);
    for (size_t k = 0; k < n && colon != std::string::npos; ++k) {
        if (key != table[k].name) continue;
        char* end = nullptr;
        errno = 0;
        char* field = reinterpret_cast<char*>(out) + table[k].offset;
        if (table[k].is_double) {
            const double v = std::strtod(value.c_str(), &end);
            if (value.empty() || *end || errno) break;
            std::memcpy(field, &v, sizeof(v));
        } else {
            const long v = std::strtol(value.c_str(), &end, 10);
            if (value.empty() || *end || errno || v < INT32_MIN || v > INT32_MAX) break;
            const int32_t v32 = (int32_t)v;
            std::memcpy(field, &v32, sizeof(v32));
        }
        return true;
    }
    bool known = false;
    for (size_t k = 0; k < n; ++k) known = known || key == table[k].name;
    *err = known && colon != std::string::npos ? "cannot read '" + value + "' as a value of " + key : "unknown key '" + key + "'";
    return false;
}

// The file at `path` over the values `out` holds.  false + `err` = "path:line: what" on the first line that cannot be read.
inline bool load(const std::string& path, limo_depth_params* out, std::string* err) {
    std::ifstream in(path);
    if (!in) {
        *err = path + ": cannot open";
        return false;
    }
    std::string line, what;
    for (int no = 1; std::getline(in, line); ++no) {
        if (no == 1 && line.compare(0, 5, "%YAML") == 0) continue;
        if (!parseLine(line, out, &what)) {
            *err = path + ":" + std::to_string(no) + ": " + what;
            return false;
        }
    }
    return true;
}

}  // namespace depth_params_yaml
}  // namespace keyframe_bundle_adjustment
