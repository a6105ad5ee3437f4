// The settings of filter_mrc and the parser of its command line (same spelling, units and defaults as
// bin/filter_mrc/settings.cpp; the flags are listed at the top of filter_mrc.cpp).
// Part of filter_mrc.cpp's one translation unit (hence the unnamed namespace).
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/visfd_hip.hpp"

namespace {

using namespace visfd;
using std::string;
using std::vector;

struct Settings {
  string in, out, mask, save_base;
  float voxel_width = -1;
  int bin = 0;                 // settings.cpp:48-49: 0 = not specified (automatic), else the factor
  bool bin_explicit = false;
  float masked_voxel_brightness = 0.0f;   // settings.cpp:41-42: voxels with mask == 0 get this value in the output
  enum { NONE, GAUSS, DOG, LOG, BLOB, BLOB_NONMAX, SURFACE_RIDGE, LOCAL_FLUCTUATIONS, MORPHOLOGY, FIND_EXTREMA, GGAUSS, DOGG, DRAW_SPHERES, WATERSHED, DISTANCE_TO_POINTS, DISTANCE_TO_VOXELS, BLOB_NONMAX_SUPERVISED_MULTI } type = NONE;
  // grayscale morphology (settings.cpp:55-57): op is a VISFD_HIP_MORPH_* code; radii in physical units until prepare() divides
  int morph_op = VISFD_HIP_MORPH_DILATE;
  float morph_r = 0.0f, morph_rmax = 0.0f, morph_bmax = 0.0f;
  // local minima / maxima (settings.cpp:97-102)
  bool find_minima = false, find_maxima = false;
  string find_minima_file, find_maxima_file;
  int neighbor_connectivity = 3;
  bool extrema_on_boundary = true;
  // watershed segmentation (settings.cpp:156-162)
  bool clusters_begin_at_maxima = false;
  float watershed_threshold = std::numeric_limits<float>::infinity();
  bool watershed_show_boundaries = true;
  float watershed_boundary_label = 0.0f;
  string watershed_markers_filename;
  float width_a[3] = {0, 0, 0}, width_b[3] = {0, 0, 0}, log_width[3] = {0, 0, 0};
  float template_background_radius[3] = {-1, -1, -1};        // settings.cpp:222-225 (-fluct)
  float template_background_exponent = 2.0f;
  float m_exp = 2.0f, n_exp = 2.0f;                           // settings.cpp:73-74 (-exponent, -exponents)
  float truncate_ratio = -1.0f, truncate_threshold = 0.03f;   // settings.cpp:81,88
  float delta = 0.02f;                                        // settings.cpp:95
  bool normalize = true;
  // blobs
  vector<float> blob_diameters;
  float blob_aspect_ratio[3] = {1.0f, 1.0f, 1.0f};            // settings.cpp:134-136, -blob-aspect-ratio
  string blob_min_file, blob_max_file;
  float score_lower = -std::numeric_limits<float>::infinity();
  float score_upper = std::numeric_limits<float>::infinity();
  bool score_bounds_are_ratios = false;                       // settings.cpp:123: -minima-ratio, -maxima-ratio (BlobDogD's ratios of the extreme score)
  float sphere_diameters_lower = -std::numeric_limits<float>::infinity();   // settings.cpp:124-125: -spheres-nonmax-radii-range; compared
  float sphere_diameters_upper = std::numeric_limits<float>::infinity();    // with the DIAMETERS in voxels as typed (handlers.cpp:547-548)
  // supervised score thresholds (settings.cpp:301-322): -auto-thresh score, -supervised POS NEG, -supervised-multi FILE
  bool auto_thresh_score = false;
  string training_pos_file, training_neg_file;
  vector<std::array<float, 3> > training_pos_crds, training_neg_crds;
  bool is_training_pos_in_voxels = false, is_training_neg_in_voxels = false;
  vector<string> multi_training_pos_files, multi_training_neg_files, multi_in_crds_files;
  vector<vector<std::array<float, 3> > > multi_training_pos_crds, multi_training_neg_crds;
  // sphere drawing (settings.cpp:107-120)
  float sphere_decals_diameter = -1.0f;
  bool sphere_decals_diameter_in_voxels = false;
  float sphere_decals_foreground = 1.0f, sphere_decals_background = 0.0f, sphere_decals_background_scale = 1.0f;
  bool sphere_decals_foreground_use_score = true, sphere_decals_background_norm = false, sphere_decals_foreground_norm = false;
  float sphere_decals_scale = 1.0f;
  float sphere_decals_shell_thickness = 1.0f, sphere_decals_shell_thickness_min = 1.0f;
  bool sphere_decals_shell_thickness_is_ratio = true;
  vector<SimpleRegion<float> > mask_regions;                  // -mask-rect, -mask-sphere and their -subtract forms, in order
  // blob list post-processing (-discard-blobs)
  vector<string> in_crds_files;
  string out_crds_file;
  string out_distances_file;                                  // -distance-to-voxels (settings.cpp:2272-2283)
  float nonmax_min_radial_separation_ratio = 0.0f;            // settings.cpp:137
  float nonmax_max_overlap_large = std::numeric_limits<float>::infinity();
  float nonmax_max_overlap_small = std::numeric_limits<float>::infinity();
  // clustering of the detected surface (-connect ...), settings.cpp:163-178
  bool cluster_connected_voxels = false;
  string must_link_filename;                       // -must-link FILE (settings.cpp:3183-3195)
  vector<float> must_link_crds;                    // flat x,y,z of every location, group after group
  vector<int64_t> must_link_group_sizes;
  vector<int> must_link_directions;                // 0 same, 1 opposite, 2 automatic (one per location)
  bool must_link_in_voxels = false;
  float connect_threshold_saliency = std::numeric_limits<float>::infinity();
  float connect_threshold_vector_saliency = (float)std::cos(M_PI * 15 / 180.0);
  float connect_threshold_vector_neighbor = (float)std::cos(M_PI * 15 / 180.0);
  float connect_threshold_tensor_saliency = (float)std::cos(M_PI * 15 / 180.0);
  float connect_threshold_tensor_neighbor = (float)std::cos(M_PI * 15 / 180.0);
  string out_normals_file;                                    // -normals-file (settings.cpp:2965-2979)
  int select_cluster = 0;                                     // settings.cpp:168
  float max_distance_to_feature = 1.3f;                       // settings.cpp:147 (voxels; negative: physical units)
  float surface_normal_curve_ds = 0.2f;                       // settings.cpp:148
  bool surface_find_ridge = true;                             // settings.cpp:149
  bool undefined_voxels_are_max = true;                       // settings.cpp:43-44
  float undefined_voxel_brightness = -1.0f;
  string load_base;
  // membranes
  bool ridges_are_maxima = false;
  float hessian_thr = 0.05f;                                  // settings.cpp:150-151
  bool hessian_thr_is_fraction = true;
  float tv_sigma = 0.0f;
  int tv_exponent = 4;                                        // settings.cpp:154
  float tv_truncate = std::sqrt(2.0);                         // settings.cpp:155
  // Z-slab run across the GPUs of a node (no reference counterpart: the reference is single-process).  One filter_mrc per GPU:
  //   VISFD_HIP_DEVICE=r filter_mrc ... -slab r WORLD IDFILE -out out_r.rec
  int slab_rank = -1, slab_world = 0;
  string slab_id_file;
  // the tail of every run (settings.cpp:34-40, :181-202): -invert, one intensity map, -rescale-min-max; -mask-select
  bool invert_output = false;
  bool use_intensity_map = false, use_dual_thresholds = false, use_rescale_multiply = false, use_gauss_thresholds = false;
  float in_threshold_01_a = 0.0f, in_threshold_01_b = 0.0f, in_threshold_10_a = 0.0f, in_threshold_10_b = 0.0f;
  bool out_thresh2_use_clipping = false, out_thresh2_use_clipping_sigma = false;
  float out_thresh_a_value = 0.0f, out_thresh_b_value = 1.0f;
  float out_thresh_gauss_x0 = 0.0f, out_thresh_gauss_sigma = 1.0f;
  float out_rescale_multiply = 1.0f, out_rescale_offset = 0.0f;
  bool rescale_min_max_out = false;
  float out_rescale_min = 0.0f, out_rescale_max = 1.0f;
  bool use_mask_select = false;
  int mask_select = 1;
  string threshold_flag;       // the last flag of the threshold family (the maps that read the input image), for messages
  string tail_flag;            // the first flag of the tail that was given (empty: none), for messages
  // the map reads the input image and overwrites the output (handlers.cpp:1044-1077); -rescale / -fill win over it
  bool threshold_map() const { return use_intensity_map && !use_rescale_multiply; }
  bool has_tail() const { return invert_output || use_intensity_map || rescale_min_max_out; }
};

bool read_must_link_file(const string& path, Settings& s);
bool parse_coordinate_line(string line, vector<float>& xyz);
bool read_coordinates(const string& path, vector<std::array<float, 3> >& crds);
void read_training_files(Settings& s);

// The one test of a numeric argument: v[i] is there, is not empty, does not start with '-' unless the number may be
// negative, and parses as a float; anything else is the error `msg`.  The reference words its messages per flag
// (typos included), so the caller passes the whole text.
float number(const vector<string>& v, size_t i, const string& msg, bool may_be_negative) {
  if (i >= v.size() || v[i].empty() || (!may_be_negative && v[i][0] == '-')) throw VisfdErr(msg);
  try { return std::stof(v[i]); } catch (...) { throw VisfdErr(msg); }
}

string after(const string& flag, const string& what) {
  return "Error: The " + flag + " argument must be followed by " + what + "\n";
}

bool one_of(const string& f, std::initializer_list<const char*> names) {
  for (const char* n : names) if (f == n) return true;
  return false;
}

Settings parse(int argc, char** argv) {
  Settings s;
  bool user_set_thickness_manually = false, user_set_background_scale_manually = false;   // settings.cpp:260-261
  bool user_set_watershed_threshold_manually = false;
  vector<string> v(argv + 1, argv + argc);
  for (size_t i = 0; i < v.size();) {
    const string& f = v[i];
    auto need = [&](size_t k) { if (i + k >= v.size()) throw VisfdErr("Error: The " + f + " argument needs " + std::to_string(k) + " parameter(s).\n"); };
    auto num = [&](size_t k) { return number(v, i + k, after(f, "a number."), true); };   // the k-th word after the flag
    if (f == "-in" || f == "-i") { need(1); s.in = v[i + 1]; i += 2; }
    else if (f == "-out" || f == "-o") { need(1); s.out = v[i + 1]; i += 2; }
    else if (f == "-mask") { need(1); s.mask = v[i + 1]; i += 2; }
    else if (f == "-w") { need(1); s.voxel_width = num(1); i += 2; }
    else if (f == "-mask-out") { need(1); s.masked_voxel_brightness = num(1); i += 2; }   // settings.cpp:662-674
    else if (f == "-np") { need(1); i += 2; }  // host threads: not used by the GPU path
    else if (f == "-bin") {
      need(1);
      const float b = num(1);
      if (b < 1.0f || b != std::floor(b)) throw VisfdErr("Error: The " + f + " argument must be followed by a positive integer.\n");
      s.bin = (int)b;              // settings.cpp:703-716
      s.bin_explicit = true;
      i += 2;
    }
    else if (f == "-gauss") { need(1); s.width_a[0] = s.width_a[1] = s.width_a[2] = num(1); s.type = Settings::GAUSS; i += 2; }
    else if (f == "-fluct" || f == "-fluctuation" || f == "-fluctuations") {     // settings.cpp:2170-2186
      need(1);
      s.template_background_radius[0] = s.template_background_radius[1] = s.template_background_radius[2] = num(1);
      s.type = Settings::LOCAL_FLUCTUATIONS; s.masked_voxel_brightness = 0.0f; i += 2;
    }
    else if (f == "-fluct-aniso" || f == "-fluctuation-aniso" || f == "-fluctuations-aniso") {   // settings.cpp:2138-2156
      need(3);
      for (int d = 0; d < 3; d++) s.template_background_radius[d] = num(1 + d);
      s.type = Settings::LOCAL_FLUCTUATIONS; s.masked_voxel_brightness = 0.0f; i += 4;
    }
    else if (f == "-dilate" || f == "-dilation" || f == "-erode" || f == "-erosion" || f == "-open" || f == "-opening" ||
             f == "-close" || f == "-closing" || f == "-top-hat-white" || f == "-top-hat-black") {
      s.morph_r = number(v, i + 1, after(f, "a nonnegative number"), false);
      s.morph_op = (f == "-dilate" || f == "-dilation") ? VISFD_HIP_MORPH_DILATE
                 : (f == "-erode" || f == "-erosion") ? VISFD_HIP_MORPH_ERODE
                 : (f == "-open" || f == "-opening") ? VISFD_HIP_MORPH_OPEN
                 : (f == "-close" || f == "-closing") ? VISFD_HIP_MORPH_CLOSE
                 : (f == "-top-hat-white") ? VISFD_HIP_MORPH_TOP_HAT_WHITE : VISFD_HIP_MORPH_TOP_HAT_BLACK;
      s.type = Settings::MORPHOLOGY; i += 2;
    }
    else if (f == "-dilate-binary-soft" || f == "-dilation-binary-soft" || f == "-erode-binary-soft" ||
             f == "-erosion-binary-soft") {
      // all three numbers are required (the reference's -dilate-binary-soft tests only two of them before reading the third)
      for (size_t k = 1; k <= 3; k++) number(v, i + k, after(f, "nonnegative numbers"), false);
      s.morph_r = number(v, i + 1, after(f, "nonnegative numbers"), false);
      s.morph_rmax = number(v, i + 2, after(f, "nonnegative numbers"), false);
      s.morph_bmax = number(v, i + 3, after(f, "nonnegative numbers"), false);
      s.morph_op = (f == "-dilate-binary-soft" || f == "-dilation-binary-soft") ? VISFD_HIP_MORPH_DILATE : VISFD_HIP_MORPH_ERODE;
      s.type = Settings::MORPHOLOGY; i += 4;
    }
    else if (f == "-find-minima" || f == "-find-maxima") {   // settings.cpp:2202-2231 (the wording is the reference's)
      if (i + 1 >= v.size()) throw VisfdErr("Error: The " + f + " argument must be followed by a number.\n");
      if (f == "-find-minima") { s.find_minima = true; s.find_minima_file = v[i + 1]; }
      else { s.find_maxima = true; s.find_maxima_file = v[i + 1]; }
      s.type = Settings::FIND_EXTREMA; i += 2;
    }
    else if (f == "-neighbor-connectivity") {   // settings.cpp:2234-2247
      const string msg = "Error: The " + f + " argument must be followed by a positive integer.\n";
      if (i + 1 >= v.size()) throw VisfdErr(msg);
      try { s.neighbor_connectivity = std::stoi(v[i + 1]); } catch (...) { throw VisfdErr(msg); }
      if (s.neighbor_connectivity <= 0) throw VisfdErr(msg);
      if (s.neighbor_connectivity > VISFD_HIP_EXTREMA_MAX_CONNECTIVITY)
        throw VisfdErr("Error: The " + f + " argument must be 1, 2 or 3 (6, 18 or 26 neighbors) in this program:\n"
                       "       larger neighborhoods are not supported on the GPU.\n");
      i += 2;
    }
    else if (f == "-boundary-extrema") { s.extrema_on_boundary = true; i += 1; }
    else if (f == "-ignore-boundary-extrema") { s.extrema_on_boundary = false; i += 1; }
    else if (f == "-watershed") {   // settings.cpp:2581-2608: the kind resets the threshold unless one was given before it
      const float inf = std::numeric_limits<float>::infinity();
      const string kind = (i + 1 < v.size() && !v[i + 1].empty() && v[i + 1][0] != '-') ? v[i + 1] : "";
      if (kind == "min" || kind == "minima") {
        s.clusters_begin_at_maxima = false;
        if (!user_set_watershed_threshold_manually) s.watershed_threshold = inf;
      } else if (kind == "max" || kind == "maxima") {
        s.clusters_begin_at_maxima = true;
        if (!user_set_watershed_threshold_manually) s.watershed_threshold = -inf;
      } else {
        // the reference's text verbatim (settings.cpp:2602-2605), its stray "width" included: the flag takes the kind only
        throw VisfdErr("Error: The " + f + " argument must be followed by an argument:  \"type\"  \"width\"\n"
                       "       The \"type\" argument must be either \"minima\" or \"maxima\".\n"
                       "       (It depends on whether you want to detect dark or bright objects.)\n");
      }
      s.type = Settings::WATERSHED; i += 2;
    }
    else if (f == "-watershed-threshold" || f == "-watershed-boundary") {   // settings.cpp:2612-2663
      const float x = number(v, i + 1, after(f, "a number"), true);
      if (f == "-watershed-threshold") { user_set_watershed_threshold_manually = true; s.watershed_threshold = x; }
      else s.watershed_boundary_label = x;
      s.type = Settings::WATERSHED; i += 2;
    }
    else if (f == "-watershed-show-boundaries") { s.watershed_show_boundaries = true; s.type = Settings::WATERSHED; i += 1; }
    else if (f == "-watershed-hide-boundaries") { s.watershed_show_boundaries = false; s.type = Settings::WATERSHED; i += 1; }
    else if (f == "-markers") {   // settings.cpp:2667-2680
      if (i + 1 >= v.size() || v[i + 1].empty())
        throw VisfdErr("Error: The " + f + " argument must be followed by an image file name\n");
      s.watershed_markers_filename = v[i + 1]; i += 2;
    }
    else if (f == "-ggauss" || f == "-ggauss-aniso" || f == "-dogg" || f == "-dogg-aniso" || f == "-exponent" ||
             f == "-gauss-exponent" || f == "-exponents" || f == "-gdog-exponents") {
      // settings.cpp:1220-1335, :1492-1535: the numbers must be there, not empty and not start with '-'
      const bool aniso = f == "-ggauss-aniso" || f == "-dogg-aniso", two = f == "-dogg" || f == "-dogg-aniso";
      const bool expo = f == "-exponent" || f == "-gauss-exponent", expos = f == "-exponents" || f == "-gdog-exponents";
      const size_t k = expo ? 1 : expos ? 2 : (aniso ? 3 : 1) * (two ? 2 : 1);
      const string msg = "Error: The " + f + " argument must be followed by " +
                         (k == 1 ? string(expo ? "a positive number.\n" : "a positive number (\"s\"),\n the Gaussian width\n")
                                 : expos ? string("two positive numbers.\n")
                                         : std::to_string(k) + " positive numbers" + (k == 3 ? ":\n s_x  s_y  s_z\n the Gaussian widths in the X, Y, and Z direction.)\n" : ".\n"));
      float x[6] = {0, 0, 0, 0, 0, 0};
      for (size_t j = 1; j <= k; j++) x[j - 1] = number(v, i + j, msg, false);
      if (expo) s.m_exp = s.n_exp = s.template_background_exponent = x[0];
      else if (expos) { s.m_exp = x[0]; s.n_exp = s.template_background_exponent = x[1]; }   // settings.cpp:1500-1503
      else {
        for (int d = 0; d < 3; d++) {
          s.width_a[d] = aniso ? x[d] : x[0];
          if (two) s.width_b[d] = aniso ? x[3 + d] : x[1];
        }
        s.type = two ? Settings::DOGG : Settings::GGAUSS;
      }
      i += k + 1;
    }
    else if (f == "-gauss-aniso") { need(3); for (int d = 0; d < 3; d++) s.width_a[d] = num(1 + d); s.type = Settings::GAUSS; i += 4; }
    else if (f == "-dog") {
      need(2);
      s.width_a[0] = s.width_a[1] = s.width_a[2] = num(1);
      s.width_b[0] = s.width_b[1] = s.width_b[2] = num(2);
      s.type = Settings::DOG; i += 3;
    }
    else if (f == "-dog-aniso") {                                                         // settings.cpp:1275-1305
      if (i + 6 >= v.size()) throw VisfdErr("Error: The " + f + " argument must be followed by 6 positive numbers.\n");
      for (int k = 1; k <= 6; k++)
        if (v[i + k].empty() || v[i + k][0] == '-') throw VisfdErr("Error: The " + f + " argument must be followed by 6 positive numbers.\n");
      for (int d = 0; d < 3; d++) { s.width_a[d] = num(1 + d); s.width_b[d] = num(4 + d); }
      s.type = Settings::DOG; i += 7;
    }
    else if (f == "-blob-aspect-ratio") {                                                 // settings.cpp:1628-1644
      need(3);
      for (int d = 0; d < 3; d++) s.blob_aspect_ratio[d] = num(1 + d);
      i += 4;
    }
    else if (f == "-log" || f == "-log-r" || f == "-log-d") {
      need(1);
      float m = 1.0f;
      if (f == "-log-r") m = (float)(1.0 / std::sqrt(3.0));
      if (f == "-log-d") m = (float)(1.0 / (2.0 * std::sqrt(3.0)));
      s.log_width[0] = s.log_width[1] = s.log_width[2] = num(1) * m;
      s.type = Settings::LOG; i += 2;
    }
    else if (f == "-log-aniso") { need(3); for (int d = 0; d < 3; d++) s.log_width[d] = num(1 + d); s.type = Settings::LOG; i += 4; }
    else if (f == "-dog-delta") { need(1); s.delta = num(1); i += 2; }
    else if (f == "-truncate") { need(1); s.truncate_ratio = num(1); s.truncate_threshold = -1.0f; i += 2; }
    else if (f == "-truncate-threshold") { need(1); s.truncate_threshold = num(1); s.truncate_ratio = -1.0f; i += 2; }
    else if (f == "-normalize-filters") {
      need(1);
      if (v[i + 1] == "no") s.normalize = false;
      else throw VisfdErr("Error: -normalize-filters accepts \"no\" only (as in the reference, settings.cpp:492-496).\n");
      i += 2;
    }
    else if (f == "-blob" || f == "-blob-sigma" || f == "-blob-s" || f == "-blobs" || f == "-blob-radii" ||
             f == "-blob-r" || f == "-blobr" || f == "-blob-diameters" || f == "-blob-d") {
      need(5);
      const string kind = v[i + 1], base = v[i + 2];
      if (kind == "minima" || kind == "min") { s.blob_min_file = base; s.blob_max_file = ""; s.score_upper = 0.0f; }
      else if (kind == "maxima" || kind == "max") { s.blob_max_file = base; s.blob_min_file = ""; s.score_lower = 0.0f; }
      else if (kind == "all") {
        s.blob_min_file = base + ".minima.txt"; s.blob_max_file = base + ".maxima.txt";
        if (s.score_lower == 0.0f) s.score_lower = -std::numeric_limits<float>::infinity();
        if (s.score_upper == 0.0f) s.score_upper = std::numeric_limits<float>::infinity();
      } else throw VisfdErr("Error: The 1st parameter to \"" + f + "\" must be \"minima\", \"maxima\" or \"all\".\n");
      const float wmin = num(3), wmax = num(4);
      float growth = num(5);
      if (wmin <= 0 || wmax <= 0 || wmin >= wmax || growth <= 1.0f)
        throw VisfdErr("Error: " + f + " needs 0 < min < max and a growth ratio > 1.\n");
      const int N = 1 + (int)std::ceil(std::log(wmax / wmin) / std::log(growth));   // settings.cpp:1719
      growth = (float)std::pow(wmax / wmin, 1.0 / N);
      float mult = 1.0f;
      if (f == "-blob-sigma" || f == "-blob-s") mult = (float)(2.0 * std::sqrt(3.0));
      if (f == "-blob-radii" || f == "-blob-r" || f == "-blobr") mult = 2.0f;
      else if (f == "-blob-diameters" || f == "-blob-d") mult = 1.0f;
      s.blob_diameters.resize((size_t)N);
      s.blob_diameters[0] = wmin * mult;
      for (int n = 1; n < N; n++) s.blob_diameters[(size_t)n] = s.blob_diameters[(size_t)n - 1] * growth;
      s.type = Settings::BLOB; i += 6;
    }
    else if (f == "-discard-blobs" || f == "-blob-nonmax" || f == "-blobs-nonmax") {   // settings.cpp:1769-1787
      need(2);
      if (v[i + 1].empty() || v[i + 1][0] == '-' || v[i + 2].empty() || v[i + 2][0] == '-' || v[i + 1] == v[i + 2])
        throw VisfdErr("Error: The " + f + " argument must be followed by two different file names\n");
      s.in_crds_files.push_back(v[i + 1]);
      s.out_crds_file = v[i + 2];
      s.type = Settings::BLOB_NONMAX;
      i += 3;
    }
    else if (f == "-radial-separation" || f == "-blob-separation" || f == "-blob-r-separation" ||
             f == "-blobr-separation" || f == "-spheres-nonmax-separation-radius") {   // settings.cpp:1603-1624
      need(1); s.nonmax_min_radial_separation_ratio = num(1); i += 2;
    }
    else if (f == "-max-volume-overlap") { need(1); s.nonmax_max_overlap_large = num(1); i += 2; }        // settings.cpp:1540
    else if (f == "-max-volume-overlap-small") { need(1); s.nonmax_max_overlap_small = num(1); i += 2; }  // settings.cpp:1561
    else if (one_of(f, {"-minima-threshold", "-score-upper-bound", "-maxima-threshold", "-score-lower-bound", "-minima-ratio",
                        "-score-lower-bound-ratio", "-maxima-ratio", "-score-upper-bound-ratio"})) {   // settings.cpp:1909-1981
      // (the -ratio spellings are the reference's: -score-lower-bound-ratio sets the UPPER bound, like -minima-ratio)
      need(1);
      const bool upper = one_of(f, {"-minima-threshold", "-score-upper-bound", "-minima-ratio", "-score-lower-bound-ratio"});
      (upper ? s.score_upper : s.score_lower) = num(1);
      s.score_bounds_are_ratios = f.size() > 6 && f.substr(f.size() - 6) == "-ratio";
      i += 2;
    }
    else if (f == "-spheres-nonmax-radii-range" || f == "-sphere-nonmax-radii-range") {   // settings.cpp:1985-1999
      const string msg = "Error: The " + f + " argument must be followed by a number number.\n";
      s.sphere_diameters_lower = number(v, i + 1, msg, false);
      s.sphere_diameters_upper = number(v, i + 2, msg, false);
      i += 3;
    }
    else if (f == "-spheres-nonmax-score-range" || f == "-sphere-nonmax-score-range") {   // settings.cpp:2003-2016
      const string msg = "Error: The " + f + " argument must be followed by two numbers.\n";
      s.score_lower = number(v, i + 1, msg, true);
      s.score_upper = number(v, i + 2, msg, true);
      i += 3;
    }
    else if (f == "-auto-thresh") {   // settings.cpp:1792-1810
      s.auto_thresh_score = true;
      if (i + 1 >= v.size() || v[i + 1] != "score")
        throw VisfdErr("Error: The " + f + " argument must be followed by \"score\"\n"
                       "       (In the future, it may be followed by a list of attributes surrounded\n"
                       "        in quotes.  But currently only the \"score\" attribute is supported.\n"
                       "        Thresholds for these attributes will be determined automatically.)\n");
      i += 2;
    }
    else if (f == "-supervised") {   // settings.cpp:1814-1830
      if (i + 2 >= v.size() || v[i + 1].empty() || v[i + 2].empty())
        throw VisfdErr("Error: The " + f + " argument must be followed by two file names:\n"
                       "       FILE_POS.txt  FILE_NEG.txt\n"
                       "       containing positive and negative training data, respectively.\n");
      s.training_pos_file = v[i + 1];
      s.training_neg_file = v[i + 2];
      i += 3;
    }
    else if (f == "-supervised-multi") {   // settings.cpp:1834-1905: a file of "pos_file neg_file blob_list_file" lines
      s.type = Settings::BLOB_NONMAX_SUPERVISED_MULTI;
      if (i + 1 >= v.size() || v[i + 1].empty())
        throw VisfdErr("Error: The " + f + " argument must be followed a file name. Example: FILE_TRAINING_SETS.txt\n"
                       "\n"
                       "File format details:\n"
                       " This should be a 3-column text file containing file names.  Example:\n"
                       "   training_pos_1.txt  training_crds_neg_1.txt  blob_info_1.txt\n"
                       "   training_pos_2.txt  training_crds_neg_2.txt  blob_info_2.txt\n"
                       "   training_pos_3.txt  training_crds_neg_3.txt  blob_info_3.txt\n"
                       "                :                        :                :\n"
                       "   training_pos_N.txt  training_crds_neg_N.txt  blob_info_N.txt\n"
                       "\n"
                       " containing positive and negative training data, and a list of detected blobs\n"
                       " for each of the N images you want to simultaneously analyze.\n");
      const string fname = v[i + 1];
      std::ifstream meta(fname.c_str());   // (a file that cannot be opened reads as empty, as in the reference)
      string line;
      size_t i_line = 1;
      while (std::getline(meta, line)) {
        const size_t hash = line.find('#');
        if (hash != string::npos) line = line.substr(0, hash);
        std::istringstream words(line);
        vector<string> tokens;
        string w;
        while (words >> w) tokens.push_back(w);
        if (tokens.empty()) continue;   // (the reference does not count such lines either)
        if (tokens.size() != 3) {
          std::ostringstream msg;
          msg << "Error: Format error in file:\n"
              << "       \"" << fname << "\", line: " << i_line << "\n"
              << "\n"
              << "       Expected 3 file names in every line in this file:\n"
              << "\n"
              << "       training_pos_file  training_neg_file  blob_info_list.txt\n";
          throw VisfdErr(msg.str());
        }
        s.multi_training_pos_files.push_back(tokens[0]);
        s.multi_training_neg_files.push_back(tokens[1]);
        s.multi_in_crds_files.push_back(tokens[2]);
      }
      i += 2;
    }
    else if (f == "-membrane" || f == "-surface-ridge") {
      need(2);
      if (v[i + 1] == "min" || v[i + 1] == "minima") s.ridges_are_maxima = false;
      else if (v[i + 1] == "max" || v[i + 1] == "maxima") s.ridges_are_maxima = true;
      else throw VisfdErr("Error: The " + f + " argument must be followed by \"minima\" or \"maxima\" and a width.\n");
      const float sigma = (float)(num(2) / std::sqrt(3.0));   // settings.cpp:2774
      s.width_a[0] = s.width_a[1] = s.width_a[2] = sigma;
      s.type = Settings::SURFACE_RIDGE; i += 3;
    }
    else if (f == "-detection-background" || f == "-membrane-background" || f == "-curve-background") {   // settings.cpp:2802-2825
      // the peak-height factor of the score loops: width (sigma, physical units) of the Gaussian whose output is the
      // background; both scores are multiplied by (image - background), handlers.cpp:1577-1605,1698-1702,1883-1887
      need(1);
      s.width_b[0] = s.width_b[1] = s.width_b[2] = num(1);
      s.type = Settings::SURFACE_RIDGE; i += 2;
    }
    else if (f == "-tv") { need(1); s.tv_sigma = num(1); i += 2; }
    else if (f == "-tv-angle-exponent") { need(1); s.tv_exponent = (int)num(1); i += 2; }
    else if (f == "-tv-truncate-ratio") { need(1); s.tv_truncate = num(1); i += 2; }   // settings.cpp:2931-2946
    else if (f == "-tv-best" || f == "-best") {
      need(1); s.hessian_thr = num(1); s.hessian_thr_is_fraction = true;
      if (!(s.hessian_thr >= 0.0f && s.hessian_thr <= 1.0f)) throw VisfdErr("Error: -tv-best needs a number between 0 and 1.\n");
      i += 2;
    }
    else if (f == "-detection-threshold") { need(1); s.hessian_thr = num(1); s.hessian_thr_is_fraction = false; i += 2; }
    else if (f == "-draw-spheres" || f == "-spheres" || f == "-draw-hollow-spheres") {   // settings.cpp:2306-2340
      if (i + 1 >= v.size() || v[i + 1].empty() || v[i + 1][0] == '-')
        throw VisfdErr("Error: The " + f + " argument must be followed by a file name\n");
      s.type = Settings::DRAW_SPHERES;
      s.in_crds_files.push_back(v[i + 1]);
      if (f == "-draw-hollow-spheres" && !user_set_thickness_manually) {
        s.sphere_decals_shell_thickness = 0.05f;
        s.sphere_decals_shell_thickness_is_ratio = true;
        s.sphere_decals_shell_thickness_min = 1.0f;
      }
      i += 2;
    }
    else if (one_of(f, {"-diameters", "-diameter", "-sphere-diameters", "-sphere-diameter", "-diameters-voxels", "-diameter-voxels",
                        "-sphere-diameters-voxels", "-sphere-diameter-voxels"})) {   // settings.cpp:2343-2378
      s.sphere_decals_diameter = number(v, i + 1, after(f, "a number"), false);
      s.sphere_decals_diameter_in_voxels = f.size() > 7 && f.substr(f.size() - 7) == "-voxels";
      i += 2;
    }
    else if (one_of(f, {"-radii", "-radius", "-sphere-radii", "-sphere-radius", "-radii-voxels", "-radius-voxels",
                        "-sphere-radii-voxels", "-sphere-radius-voxels"})) {         // settings.cpp:2381-2416
      s.sphere_decals_diameter = (float)(number(v, i + 1, after(f, "a number"), false) * 2.0);
      s.sphere_decals_diameter_in_voxels = f.size() > 7 && f.substr(f.size() - 7) == "-voxels";
      i += 2;
    }
    else if (f == "-spheres-scale" || f == "-sphere-scale") {                        // settings.cpp:2419-2434
      s.sphere_decals_scale = number(v, i + 1, after(f, "a number:\n"
                    "       the ratio of the displyed sphere size to the diameter detected (usually 1)."), false);
      i += 2;
    }
    else if (f == "-sphere-shell-ratio" || f == "-spheres-shell-ratio") {            // settings.cpp:2437-2453
      s.sphere_decals_shell_thickness = number(v, i + 1, after(f, "a numbers:\n"
                    "       -the ratio of the shell thickness to the sphere diameter"), false);
      s.sphere_decals_shell_thickness_is_ratio = true;
      user_set_thickness_manually = true;
      i += 2;
    }
    else if (one_of(f, {"-sphere-shell-thickness-min", "-sphere-shell-thicknesses-min", "-spheres-shell-thickness-min",
                        "-spheres-shell-thicknesses-min"})) {                         // settings.cpp:2456-2472
      s.sphere_decals_shell_thickness_min = number(v, i + 1, after(f, "a number"), false);
      user_set_thickness_manually = true;
      i += 2;
    }
    else if (one_of(f, {"-sphere-shell-thickness", "-sphere-shell-thicknesses", "-spheres-shell-thickness",
                        "-spheres-shell-thicknesses"})) {                             // settings.cpp:2475-2492
      s.sphere_decals_shell_thickness = number(v, i + 1, after(f, "a number"), false);
      s.sphere_decals_shell_thickness_is_ratio = false;
      user_set_thickness_manually = true;
      i += 2;
    }
    else if (f == "-spheres-score" || f == "-sphere-score") { s.sphere_decals_foreground_use_score = true; i += 1; }
    else if (f == "-background" || f == "-spheres-background" || f == "-sphere-background") {   // settings.cpp:2502-2518
      s.sphere_decals_background_scale = 0.0f;
      s.sphere_decals_background = number(v, i + 1, after(f, "a number:\n"
                    "       the voxel intensity value outside the sphere (normally 0)."), true);
      i += 2;
    }
    else if (f == "-background-scale" || f == "-spheres-background-scale" || f == "-sphere-background-scale") {   // :2521-2538
      s.sphere_decals_background_scale = number(v, i + 1, after(f, "a number, usually between 0 and 1:\n"
                    "       how much to supress fluctuations in the original background image."), false);
      user_set_background_scale_manually = true;
      i += 2;
    }
    else if (f == "-foreground" || f == "-spheres-foreground" || f == "-sphere-foreground") {   // settings.cpp:2541-2556
      s.sphere_decals_foreground_use_score = false;
      s.sphere_decals_foreground = number(v, i + 1, after(f, "a number:\n"
                    "       the voxel intensity value on the sphere (normally 1)."), true);
      i += 2;
    }
    else if (f == "-background-auto") {                                              // settings.cpp:2558-2564
      s.sphere_decals_background_norm = true;
      if (!user_set_background_scale_manually) s.sphere_decals_background_scale = 0.3f;
      i += 1;
    }
    else if (f == "-spheres-normalize" || f == "-sphere-normalize") { s.sphere_decals_foreground_norm = true; i += 1; }
    else if (one_of(f, {"-spheres01", "-spheres-01", "-sphere01", "-sphere-01"})) { s.sphere_decals_foreground_norm = false; i += 1; }
    else if (f == "-distance-points") {                                                // settings.cpp:2262-2269
      if (i + 1 >= v.size()) throw VisfdErr("Error: The " + f + " argument must be followed by a file name.\n");
      s.type = Settings::DISTANCE_TO_POINTS;
      s.in_crds_files.push_back(v[i + 1]);
      i += 2;
    }
    else if (f == "-distance-to-voxels") {                                             // settings.cpp:2272-2283
      const string msg = "Error: The " + f + " argument must be followed by two file names and two numbers:\n"
                         "       InFile OutFile BrightnessSelectMin BrightnessSelectMax\n";
      if (i + 4 >= v.size()) throw VisfdErr(msg);
      s.type = Settings::DISTANCE_TO_VOXELS;
      s.in_crds_files.push_back(v[i + 1]);
      s.out_distances_file = v[i + 2];
      try { s.out_thresh_a_value = std::stof(v[i + 3]); s.out_thresh_b_value = std::stof(v[i + 4]); }
      catch (...) { throw VisfdErr(msg); }
      i += 5;
    }
    else if (f == "-random-spheres")
      throw VisfdErr("Error: -random-spheres is not provided by this program (it needs the reference's random numbers).\n");
    else if (one_of(f, {"-mask-rect", "-mask-rectangle", "-mask-rect-subtract", "-mask-rectangle-subtract", "-mask-sphere",
                        "-mask-sphere-subtract"})) {                                   // settings.cpp:519-633
      const bool sphere = f.find("sphere") != string::npos, subtract = f.find("subtract") != string::npos;
      const size_t k = sphere ? 4 : 6;
      const string msg = after(f, string(sphere ? "4" : "6") + " numbers.");
      float x[6] = {0, 0, 0, 0, 0, 0};
      for (size_t j = 1; j <= k; j++) x[j - 1] = number(v, i + j, msg, true);
      SimpleRegion<float> region;
      region.value = subtract ? -1.0f : 1.0f;
      if (sphere) {
        region.type = SimpleRegion<float>::SPHERE;
        region.data.sphere.x0 = x[0]; region.data.sphere.y0 = x[1]; region.data.sphere.z0 = x[2]; region.data.sphere.r = x[3];
      } else {
        region.type = SimpleRegion<float>::RECT;
        region.data.rect.xmin = x[0]; region.data.rect.xmax = x[1]; region.data.rect.ymin = x[2];
        region.data.rect.ymax = x[3]; region.data.rect.zmin = x[4]; region.data.rect.zmax = x[5];
      }
      s.mask_regions.push_back(region);
      i += k + 1;
    }
    else if (one_of(f, {"-mask-crds-units", "-mask-coords-units", "-mask-coordinates-units", "-mask-rect-units"})) {
      // settings.cpp:637-658: the reference reads the word and, its two tests being unsatisfiable, changes nothing:
      // mask coordinates are always voxels
      need(1); i += 2;
    }
    // ---- the tail: settings.cpp:954-1186 (texts verbatim) and :502-515 ----
    else if (f == "-rescale" || f == "-thresh-range" || f == "-thresh-range-out" || f == "-rescale-min-max") {
      const string msg = after(f, "2 numbers:\n outA  outB\n"
                                  "  (the desired minimum and maximum voxel intensity values for the final image)");
      const float x = number(v, i + 1, msg, true), y = number(v, i + 2, msg, true);
      if (f == "-rescale") { s.use_intensity_map = s.use_rescale_multiply = true; s.out_rescale_multiply = x; s.out_rescale_offset = y; }
      else if (f == "-rescale-min-max") { s.rescale_min_max_out = true; s.out_rescale_max = x; s.out_rescale_min = y; }   // the first is the maximum
      else { s.out_thresh_a_value = x; s.out_thresh_b_value = y; }
      if (s.tail_flag.empty()) s.tail_flag = f;
      i += 3;
    }
    else if (f == "-fill") {
      s.out_rescale_offset = number(v, i + 1, "Error: The " + f + " argument must be followed by a number.", true);
      s.use_intensity_map = s.use_rescale_multiply = true;
      s.out_rescale_multiply = 0.0f;
      if (s.tail_flag.empty()) s.tail_flag = f;
      i += 2;
    }
    else if (f == "-no-rescale" || f == "-norescale") {
      s.rescale_min_max_out = false; s.in_threshold_01_a = s.in_threshold_01_b = 1.0f; i += 1;
    }
    else if (f == "-invert" || f == "-inv") { s.invert_output = true; if (s.tail_flag.empty()) s.tail_flag = f; i += 1; }
    else if (f == "-thresh" || f == "-thresh-out") {
      s.in_threshold_01_a = s.in_threshold_01_b = number(v, i + 1, after(f, "1 number."), true);
      s.use_intensity_map = true; s.use_dual_thresholds = false;
      s.threshold_flag = f; if (s.tail_flag.empty()) s.tail_flag = f;
      i += 2;
    }
    else if (f == "-thresh2" || f == "-thresh2-out" || f == "-clip" || f == "-cl") {
      const string msg = after(f, "2 numbers.");
      const float x = number(v, i + 1, msg, true), y = number(v, i + 2, msg, true);
      s.use_intensity_map = true; s.use_dual_thresholds = false;
      s.in_threshold_01_a = x; s.in_threshold_01_b = y;
      s.out_thresh2_use_clipping = f == "-clip" || f == "-cl";
      if (s.out_thresh2_use_clipping) s.out_thresh2_use_clipping_sigma = f == "-cl";
      s.threshold_flag = f; if (s.tail_flag.empty()) s.tail_flag = f;
      i += 3;
    }
    else if (f == "-thresh4" || f == "-thresh4-out") {
      const string msg = after(f, "4 numbers\n       (These numbers must be either in increasing or decreasing order.)");
      float x[4];
      for (size_t k = 0; k < 4; k++) x[k] = number(v, i + 1 + k, msg, true);
      if (!((x[0] <= x[1] && x[1] <= x[2] && x[2] <= x[3]) || (x[0] >= x[1] && x[1] >= x[2] && x[2] >= x[3]))) throw VisfdErr(msg);
      s.use_intensity_map = s.use_dual_thresholds = true;
      s.in_threshold_01_a = x[0]; s.in_threshold_01_b = x[1]; s.in_threshold_10_a = x[2]; s.in_threshold_10_b = x[3];
      s.threshold_flag = f; if (s.tail_flag.empty()) s.tail_flag = f;
      i += 5;
    }
    else if (f == "-thresh-interval" || f == "-thresh-interval-out" || f == "-thresh-gauss" || f == "-thresh-gauss-out") {
      const string msg = after(f, "4 numbers.");   // (the reference's count; both flags take two)
      const float x = number(v, i + 1, msg, true), y = number(v, i + 2, msg, true);
      s.use_intensity_map = true;
      if (f == "-thresh-interval" || f == "-thresh-interval-out") {
        s.use_dual_thresholds = true;
        s.in_threshold_01_a = s.in_threshold_01_b = x; s.in_threshold_10_a = s.in_threshold_10_b = y;
      } else { s.use_gauss_thresholds = true; s.out_thresh_gauss_x0 = x; s.out_thresh_gauss_sigma = y; }
      s.threshold_flag = f; if (s.tail_flag.empty()) s.tail_flag = f;
      i += 3;
    }
    else if (f == "-mask-select") {
      const string msg = after(f, "an integer.");
      if (i + 1 >= v.size() || v[i + 1].empty()) throw VisfdErr(msg);
      try { s.mask_select = std::stoi(v[i + 1]); } catch (...) { throw VisfdErr(msg); }
      s.use_mask_select = true;
      if (s.tail_flag.empty()) s.tail_flag = f;
      i += 2;
    }
    else if (f == "-slab") {
      need(3);
      s.slab_rank = (int)num(1); s.slab_world = (int)num(2); s.slab_id_file = v[i + 3];
      if (s.slab_world < 1 || s.slab_rank < 0 || s.slab_rank >= s.slab_world)
        throw VisfdErr("Error: -slab RANK WORLD IDFILE needs 0 <= RANK < WORLD.\n");
      i += 4;
    }
    else if (f == "-save-progress") { need(1); s.save_base = v[i + 1]; i += 2; }
    else if (f == "-load-progress") { need(1); s.load_base = v[i + 1]; i += 2; }
    // (-connect-dark differs from -connect only in clusters_begin_at_maxima, settings.cpp:3057-3060, a flag that nothing on
    //  the membrane path reads: handlers.cpp:1341 is its only use, in the watershed handler)
    else if (f == "-connect" || f == "-connect-bright" || f == "-connect-saliency" || f == "-connect-dark") {   // settings.cpp:3036-3072
      need(1); s.cluster_connected_voxels = true; s.connect_threshold_saliency = num(1); i += 2;
    }
    else if (f == "-connect-angle") {                                                    // settings.cpp:3075-3094
      need(1); s.cluster_connected_voxels = true;
      const double theta = num(1);
      const float c = (float)std::cos(theta * M_PI / 180.0);
      s.connect_threshold_vector_saliency = s.connect_threshold_vector_neighbor = c;
      s.connect_threshold_tensor_saliency = s.connect_threshold_tensor_neighbor = c;
      i += 2;
    }
    else if (f == "-must-link") { need(1); s.must_link_filename = v[i + 1]; i += 2; }
    else if (f == "-connect-vector-saliency") { need(1); s.cluster_connected_voxels = true; s.connect_threshold_vector_saliency = num(1); i += 2; }
    else if (f == "-connect-vector-neighbor") { need(1); s.cluster_connected_voxels = true; s.connect_threshold_vector_neighbor = num(1); i += 2; }
    else if (f == "-connect-tensor-saliency") { need(1); s.cluster_connected_voxels = true; s.connect_threshold_tensor_saliency = num(1); i += 2; }
    else if (f == "-connect-tensor-neighbor") { need(1); s.cluster_connected_voxels = true; s.connect_threshold_tensor_neighbor = num(1); i += 2; }
    else if (f == "-undefined-out") {                                                    // settings.cpp:2683-2700
      need(1);
      if (v[i + 1] == "max") s.undefined_voxels_are_max = true;
      else { s.undefined_voxels_are_max = false; s.undefined_voxel_brightness = num(1); }
      i += 2;
    }
    else if (f == "-select-cluster") {                                                     // settings.cpp:3163-3182
      need(1); s.select_cluster = (int)num(1); s.cluster_connected_voxels = true;
      if (s.select_cluster < 0) throw VisfdErr("Error: The " + f + " argument must be followed by a positive integer.\n");
      i += 2;
    }
    else if (f == "-normals-file" || f == "-surface-normals-file") { need(1); s.out_normals_file = v[i + 1]; i += 2; }
    else if (f == "-max-voxels-to-feature" || f == "-max-voxels-to-surface" || f == "-max-voxels-to-membrane") {   // settings.cpp:2983-3005
      need(1);
      const string a = v[i + 1];
      s.max_distance_to_feature = (a == "inf" || a == "infinity" || a == "disable") ? 0.0f : num(1);
      i += 2;
    }
    else if (f == "-max-distance-to-feature" || f == "-max-distance-to-surface" || f == "-max-distance-to-membrane") {   // :3010-3032
      need(1);
      const string a = v[i + 1];
      s.max_distance_to_feature = (a == "inf" || a == "infinity" || a == "disable") ? 0.0f : -num(1);
      i += 2;
    }
    else throw VisfdErr("Error: Unrecognized (or unsupported on the GPU hot path) argument: \"" + f + "\"\n");
  }
  if (s.in.empty()) throw VisfdErr("Error: You must specify an input file (-in).\n");
  if (s.slab_world > 0 && (s.type == Settings::DRAW_SPHERES || !s.mask_regions.empty() || (s.type == Settings::BLOB && !s.out.empty())))
    throw VisfdErr("Error: -slab does not draw: -draw-spheres, the -mask-rect / -mask-sphere flags and \"-blob ... -out\"\n"
                   "       need the whole image in one process.\n");
  if (s.slab_world > 0 && (s.type == Settings::DISTANCE_TO_POINTS || s.type == Settings::DISTANCE_TO_VOXELS))
    throw VisfdErr(string("Error: -slab does not combine with ") +
                   (s.type == Settings::DISTANCE_TO_POINTS ? "-distance-points" : "-distance-to-voxels") +
                   ": a distance map needs the whole image in one process.\n");
  if (s.slab_world > 0 && !s.tail_flag.empty())
    throw VisfdErr("Error: -slab runs with -gauss, -blob and -membrane ... -tv alone: " + s.tail_flag + " (like every flag of\n"
                   "       -invert, the intensity maps, -rescale-min-max and -mask-select) needs the whole image in one process.\n");
  if (s.type == Settings::SURFACE_RIDGE && s.threshold_map())
    throw VisfdErr("Error: " + s.threshold_flag + " does not combine with -membrane: it maps the INPUT image, which the reference\n"
                   "       has overwritten on that path (handlers.cpp:1932, :2398).  Of the intensity maps, -membrane runs\n"
                   "       take -rescale, -fill, -invert and -rescale-min-max, which act on the output.\n");
  if (s.slab_world > 0 && s.score_bounds_are_ratios)
    throw VisfdErr("Error: -slab takes absolute score thresholds only (-minima-threshold, -maxima-threshold): a ratio of the\n"
                   "       extreme score (-minima-ratio, -maxima-ratio) needs the blobs of the whole image in one process.\n");
  if (!s.must_link_filename.empty()) s.must_link_in_voxels = read_must_link_file(s.must_link_filename, s);
  read_training_files(s);
  if (s.type == Settings::SURFACE_RIDGE) s.tv_sigma *= s.width_a[0];   // settings.cpp:3535-3540
  if (s.cluster_connected_voxels && s.type != Settings::SURFACE_RIDGE)
    throw VisfdErr("Error: this build clusters voxels (-connect) only after \"-membrane ... -tv ...\".\n");
  if (s.cluster_connected_voxels && s.connect_threshold_saliency == std::numeric_limits<float>::infinity())
    throw VisfdErr("Error: clustering needs a saliency threshold (-connect THRESHOLD).\n");
  if (!s.out_normals_file.empty() && !s.cluster_connected_voxels)
    throw VisfdErr("Error: this build writes surface normals (-normals-file) for a clustered surface only (-connect).\n");
  if ((s.cluster_connected_voxels || !s.load_base.empty()) && !(s.tv_sigma > 0))
    throw VisfdErr("Error: -connect and -load-progress need tensor voting (-tv).\n");
  return s;
}

// One line of a coordinate file (IMODWords2Crds, bin/filter_mrc/file_io.hpp:82-214): the numbers of the line, text after
// '#' ignored.  IMOD's notation -- "Pixel (x, y, z) = value" or any line whose numbers sit in parentheses -- means 1-based
// voxel indices: the first three become floor(x) - 1, and what follows "Pixel (...)" is dropped.  Returns whether the line
// was in that notation.
bool parse_coordinate_line(string line, vector<float>& xyz) {
  const size_t hash = line.find('#');
  if (hash != string::npos) line = line.substr(0, hash);
  bool parens = false, imod = false;
  for (size_t k = 0; k < line.size(); k++) {
    if (line[k] == '(' || line[k] == ')') { parens = true; line[k] = ' '; }
    else if (line[k] == ',') line[k] = ' ';
  }
  std::istringstream ws(line);
  vector<string> words;
  string w;
  while (ws >> w) words.push_back(w);
  if (!words.empty() && words[0] == "Pixel") { imod = parens = true; words.erase(words.begin()); }
  xyz.clear();
  for (size_t d = 0; d < words.size(); d++) {
    if (d >= 3 && imod) break;                       // "= value" of IMOD's line
    std::istringstream num(words[d]);
    float x;
    if (!(num >> x)) throw VisfdErr("Error: File read error (invalid entry?) on line:\n      " + line + "\n");
    if (parens && xyz.size() < 3) x = std::floor(x) - 1.0f;   // IMOD counts voxels from 1
    xyz.push_back(x);
  }
  return parens;
}

// ReadCoordinates, bin/filter_mrc/file_io.hpp:362-398: a list of locations, one per line, plain ("90.3 117.7 230") or in
// IMOD's notation (parse_coordinate_line); lines without numbers are skipped.  Returns whether any line was in voxels.
bool read_coordinates(const string& path, vector<std::array<float, 3> >& crds) {
  std::ifstream f(path.c_str());
  if (!f) throw VisfdErr("Error: unable to open \"" + path + "\" for reading.\n");
  bool in_voxels = false;
  crds.clear();
  string line;
  size_t i_line = 0;
  while (std::getline(f, line)) {
    i_line++;
    vector<float> xyz;
    in_voxels = parse_coordinate_line(line, xyz) || in_voxels;
    if (xyz.empty()) continue;
    if (xyz.size() < 3) {
      std::ostringstream msg;
      msg << "Format error near line " << i_line << " of file \"" << path << "\"\n";
      throw VisfdErr(msg.str());
    }
    std::array<float, 3> c = {{xyz[0], xyz[1], xyz[2]}};
    crds.push_back(c);
  }
  return in_voxels;
}

// settings.cpp:3556-3623: the training files of -supervised and -supervised-multi, and the two refusals of the latter
void read_training_files(Settings& s) {
  if (!s.training_pos_file.empty()) s.is_training_pos_in_voxels = read_coordinates(s.training_pos_file, s.training_pos_crds);
  if (!s.training_neg_file.empty()) s.is_training_neg_in_voxels = read_coordinates(s.training_neg_file, s.training_neg_crds);
  if (s.multi_training_pos_files.empty() && s.multi_training_neg_files.empty()) return;
  if (!s.in_crds_files.empty() && !s.out_crds_file.empty())
    throw VisfdErr("Error: This program is too stupid to automatically discard blobs from multiple\n"
                   "       images in a single invocation.  For this reason,\n"
                   "       you may not use the \"-supervised-multi\" argument simultaneously with\n"
                   "       any other arguments which also perform nonmax-suppression of blobs\n"
                   "       (such as \"-discard-blobs\").  In particular, you must make sure that\n"
                   "       any overlapping blobs in any of the reference lists of blobs must be\n"
                   "       removed in advance.  (These blobs are contained in the files referred\n"
                   "       to in the 3rd column of the file supplied to \"-supervised-multi\".\n"
                   "       They can be removed by using this program with\"-discard-blobs\"\n"
                   "       together with \"-radial-separation\", or \"-max-volume-overlap\", and/or\n"
                   "       \"-max-volume-overlap-small\".  This must be done separately\n"
                   "       for each of those files in the 3rd column.)\n");
  if (!s.mask.empty())
    throw VisfdErr("Error: You may not use the \"-supervised-multi\" argument simultaneously with\n"
                   "       the \"-mask\" argument.  If you wish to ignore blobs which lie outside\n"
                   "       the mask, then you must delete the corresponding lines from the\n"
                   "       blob lists beforehand.  (These are stored in the files indicated\n"
                   "       by the 3rd column of the file supplied to \"-supervised-multi\"\n"
                   "       You can do this by running this program using the \"-discard-blobs\"\n"
                   "       together with the \"-mask\" argument.  This must be done separately\n"
                   "       on each of these lists of blobs beforehand.)\n");
  // THE ONE DEVIATION: the reference rescales the multi sets' coordinates in loops bounded by the sizes of the -supervised
  // lists (filter_mrc.cpp:354-370).  With -supervised-multi alone those loops do nothing -- the coordinates are used as
  // read, and so they are here -- but together with -supervised they index past the multi arrays.  Refused.
  if (!s.training_pos_file.empty() || !s.training_neg_file.empty())
    throw VisfdErr("Error: -supervised-multi does not combine with -supervised: the reference rescales the multi sets'\n"
                   "       coordinates with the sizes of the -supervised lists and reads past its arrays there.\n");
  const size_t n_sets = s.multi_training_pos_files.size();
  s.multi_training_pos_crds.resize(n_sets);
  s.multi_training_neg_crds.resize(n_sets);
  for (size_t I = 0; I < n_sets; I++) {
    read_coordinates(s.multi_training_pos_files[I], s.multi_training_pos_crds[I]);
    read_coordinates(s.multi_training_neg_files[I], s.multi_training_neg_crds[I]);
  }
}

// The -must-link file (bin/filter_mrc/file_io.hpp:82-214, :667-747): groups of locations separated by blank lines; a
// line holds x y z and optionally a fourth number (> 0: the two surfaces face the same way, < 0: opposite, else
// automatic); text after '#' is ignored.  IMOD's notation -- "Pixel (x, y, z) = value" or any line whose numbers sit in
// parentheses -- means 1-based voxel indices: floor(x) - 1.  Returns whether the coordinates are voxels already.
bool read_must_link_file(const string& path, Settings& s) {
  std::ifstream f(path.c_str());
  if (!f) throw VisfdErr("Error: unable to open \"" + path + "\" for reading.\n");
  bool imod_any = false;
  vector<std::array<float, 3> > group;
  vector<int> group_dirs;
  auto close_group = [&]() {
    if (group.empty()) return;
    if (group.size() < 2 || group[0] == group[1])
      throw VisfdErr("Error: Format error in file \"" + path + "\".\n"
                     "       Each group must contain at least 2 voxels.  (Voxels appear on different\n"
                     "       lines, so blank-line delimters must not separate SINGLE non-blank lines)\n"
                     "       Furthermore, the voxels in each set must be unique.\n");
    s.must_link_group_sizes.push_back((int64_t)group.size());
    for (size_t k = 0; k < group.size(); k++) {
      for (int d = 0; d < 3; d++) s.must_link_crds.push_back(group[k][d]);
      s.must_link_directions.push_back(group_dirs[k]);
    }
    group.clear();
    group_dirs.clear();
  };
  string line;
  while (std::getline(f, line)) {
    vector<float> xyz;
    imod_any = parse_coordinate_line(line, xyz) || imod_any;
    if (xyz.empty()) { close_group(); continue; }
    if (xyz.size() != 3 && xyz.size() != 4)
      throw VisfdErr("Error: Each line of file \"" + path + "\"\n       should contain either 3 numbers, 4 numbers, or 0 numbers.\n");
    std::array<float, 3> c = {{xyz[0], xyz[1], xyz[2]}};
    group.push_back(c);
    group_dirs.push_back(xyz.size() == 4 ? (xyz[3] > 0 ? 0 : (xyz[3] < 0 ? 1 : 2)) : 2);
  }
  close_group();
  if (s.must_link_group_sizes.empty())
    throw VisfdErr("Error: Format error in file \"" + path + "\".\n       File contains no voxel coordinates.\n");
  return imod_any;
}

}  // namespace
