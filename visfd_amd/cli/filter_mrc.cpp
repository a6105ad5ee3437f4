// filter_mrc (MI355X edition) -- the hot-path subset of the reference's filter_mrc command line,
// running on libvisfd_hip.so through the visfd:: shim (include/visfd_hip.hpp).
//
// Supported flags (same spelling, units and defaults as bin/filter_mrc/settings.cpp; all lengths are
// in PHYSICAL units and are divided by the voxel width, filter_mrc.cpp:297-336):
//   -in F | -i F        input tomogram (MRC modes 0,1,2,6)
//   -out F | -o F       output tomogram (always written as mode 2, like mrc_simple.cpp:373)
//   -mask F             mask tomogram (voxels with 0 are ignored)
//   -w WIDTH            voxel width (otherwise cellA[0]/nx from the header, handlers.cpp:2429)
//   -gauss S | -gauss-aniso SX SY SZ              (settings.cpp:1220-1271, HandleGauss)
//   -dog A B                                        (settings.cpp:1309-1335, HandleDog)
//   -ggauss S | -ggauss-aniso SX SY SZ | -dogg A B | -dogg-aniso AX AY AZ BX BY BZ   (HandleGGauss, HandleDogg: the dense filter)
//   -exponent M | -gauss-exponent M | -exponents M N | -gdog-exponents M N   (settings.cpp:1492-1535; also -fluct's exponent)
//   -log S | -log-r R | -log-d D | -log-aniso SX SY SZ | -dog-delta D   (HandleLoGDoG)
//   -blob|-blob-s|-blob-r|-blob-d TYPE FILE MIN MAX GROWTH             (settings.cpp:1648-1764)
//   -minima-threshold T | -maxima-threshold T                          (settings.cpp:1915,1934)
//   -membrane {minima|maxima} THICKNESS | -surface-ridge ...           (settings.cpp:2734-2799)
//   -tv RATIO | -tv-angle-exponent N | -tv-truncate R | -tv-best F | -detection-threshold T
//   -save-progress BASE        writes BASE_tensor_{0..5}.rec           (handlers.cpp:1897-1922)
//   -truncate R | -truncate-threshold T | -normalize-filters no | -bin 1 | -np N (ignored)
//   -dilate|-dilation R | -erode|-erosion R | -open|-opening R | -close|-closing R | -top-hat-white R | -top-hat-black R
//   -dilate-binary-soft|-dilation-binary-soft R RMAX BMAX | -erode-binary-soft|-erosion-binary-soft R RMAX BMAX
//                                                                      (settings.cpp:722-915, handlers.cpp:41-145)
//   -find-minima FILE | -find-maxima FILE (both may be given) | -neighbor-connectivity N (1, 2 or 3) |
//   -boundary-extrema | -ignore-boundary-extrema                       (settings.cpp:2202-2259, HandleExtrema)
//   -draw-spheres|-spheres FILE | -draw-hollow-spheres FILE            (settings.cpp:2306-2340, HandleDrawSpheres)
//   -diameters|-radii D (and -diameter, -sphere-diameter(s), -radius, -sphere-radius|-radii; "-voxels" forms: D is in voxels)
//   -spheres-scale R | -sphere-shell-ratio R | -sphere-shell-thickness T | -sphere-shell-thickness-min T | -spheres-score
//   -background B | -background-scale S | -background-auto | -foreground F | -spheres-normalize | -spheres01
//                                                                      (settings.cpp:2343-2577; -random-spheres is not provided)
//   -blob ... -out FILE        also draws the blobs found over the input image (handlers.cpp:933-978)
//   -mask-rect XMIN XMAX YMIN YMAX ZMIN ZMAX | -mask-sphere X0 Y0 Z0 R | their -subtract forms   (settings.cpp:519-633,
//                              filter_mrc.cpp:220-286; coordinates in voxels) | -mask-crds-units UNITS (read and, as in the
//                              reference, without effect: settings.cpp:637-658)
//   -find-minima / -find-maxima with -diameters D -radial-separation R: extrema closer than that are thinned (handlers.cpp:1165-1211)
//   -invert|-inv | -thresh T | -thresh2 A B | -thresh4 A B C D | -thresh-interval A B | -thresh-gauss X0 SIGMA (each also
//   as -...-out) | -thresh-range|-thresh-range-out OUTA OUTB | -clip A B | -cl A B (in standard deviations about the mean) |
//   -rescale M O | -fill V | -rescale-min-max MAX MIN | -no-rescale|-norescale | -mask-select V
//                              the tail of every run (settings.cpp:954-1186, filter_mrc.cpp:746-786, HandleThresholds);
//                              the threshold family maps the INPUT image, as in the reference
//   -distance-points FILE (may be repeated: the files' points are appended) | -distance-to-voxels PTS OUT A B
//                              exact distance maps (settings.cpp:2262-2283, HandleDistanceToPoints,
//                              HandleDistancePointsToFeature); nx + ny + nz <= 46340; not under -slab
//   -auto-thresh score -supervised POS NEG      with -discard-blobs: after the overlap step, the score interval that
//                              misclassifies the fewest of the training points (files of locations, plain or in IMOD's
//                              notation) is chosen and the blobs outside it are discarded (settings.cpp:1792-1830,
//                              handlers.cpp:598-621); one without the other does nothing, as in the reference
//   -supervised-multi FILE     FILE lists "pos_file neg_file blob_list_file" per image: the interval that suits all sets is
//                              printed (HandleBlobScoreSupervisedMulti).  The training coordinates are used as read (the
//                              reference's rescaling loops do nothing here, filter_mrc.cpp:354-370).  Not with -discard-blobs
//                              or -mask (the reference's refusals) and -- the one deviation -- not with -supervised, where
//                              the reference reads past its arrays
//   -spheres-nonmax-radii-range A B | -spheres-nonmax-score-range A B (also -sphere-...)   bounds of -discard-blobs' first
//                              filter; the radii range is compared with the diameters in voxels as typed (handlers.cpp:547)
//   -score-upper-bound T | -score-lower-bound T   other spellings of -minima-threshold and -maxima-threshold
//   -minima-ratio R | -maxima-ratio R | -score-lower-bound-ratio R | -score-upper-bound-ratio R   -blob's thresholds as
//                              ratios of the extreme score (settings.cpp:1947-1981); not under -slab
//   The search behind the supervised flags (FindSpheres) walks the pairs on the host for small lists and runs on the GPU
//   from FIND_SPHERES_MIN_PAIRS pairs on (VISFD_HIP_FIND_SPHERES_MIN_PAIRS overrides; 0: always the GPU).
//   The overlap removal behind -discard-blobs and behind -find-minima / -find-maxima with -radial-separation
//   (DiscardOverlappingBlobs) walks the list on the host below DISCARD_OVERLAP_MIN_BLOBS blobs and runs on the GPU, when
//   there is one, from there on (VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS overrides; 0: always the GPU); same bytes either way.
// Anything else is rejected, as the reference rejects unknown arguments (settings.cpp:3340-3365).
//
// MRC input/output is in mrc.hpp, the settings and the parser of the flags above in settings.hpp; both are part of
// this translation unit and bring the shim (include/visfd_hip.hpp) and the containers with them.
#include <chrono>
#include <cstdio>
#include <ctime>
#include <iostream>
#include <sys/stat.h>
#include <thread>

#include "mrc.hpp"
#include "settings.hpp"

using std::cerr;

namespace {

// What the handlers work on, as load() and prepare() leave it
struct Run {
  const Settings& s;           // lengths in voxels once prepare() has run
  Mrc tomo_in, mask, tomo_out;
  int size[3];                 // of the image the filters see (after binning)
  float vw[3];                 // its voxel width
  int bin = 1;
  int size_orig[3];            // size and cell of the input before binning
  float cella_orig[3];
  float ratio = 0;             // where the Gaussians are truncated, in sigmas
  explicit Run(const Settings& settings) : s(settings) {}
  // the mask, null when there is none: as the 3-D table of the visfd:: calls and as the flat array of the C ABI
  float const* const* const* mask3d() const { return mask.loaded ? mask.a : nullptr; }
  const float* mask_flat() const { return mask.loaded ? &mask.a[0][0][0] : nullptr; }
};

// Blob list file (bin/filter_mrc/file_io.hpp:413-493): 3-5 numbers per line (x y z [diameter [score]]), '#'
// starts a comment; coordinates written IMOD-style in parentheses mean "units of voxels".  Returns that flag.
// imod_from_one: the coordinates of a line with parentheses become floor(x) - 1, as the reference's reader leaves them
// (file_io.hpp:201-204: IMOD counts voxels from 1); the distance handlers ask for it.
bool read_blob_file(const string& path, vector<std::array<float, 3> >& crds, vector<float>& diameters,
                    vector<float>& scores, float score_default, float diameter_factor, bool imod_from_one = false) {
  std::ifstream f(path.c_str());
  if (!f) throw VisfdErr("Error: unable to open \"" + path + "\" for reading.\n");
  bool parens = false;
  string line;
  size_t i_line = 0;
  while (std::getline(f, line)) {
    const size_t hash = line.find('#');
    if (hash != string::npos) line.erase(hash);
    bool line_parens = false;
    for (size_t k = 0; k < line.size(); k++) {
      if (line[k] == '(' || line[k] == ')') { parens = line_parens = true; line[k] = ' '; }
      else if (line[k] == ',') line[k] = ' ';
    }
    std::istringstream in(line);
    vector<float> nums;
    string tok;
    while (in >> tok) {
      try { nums.push_back(std::stof(tok)); } catch (...) { /* words such as "Pixel" or "=" are skipped */ }
    }
    if (nums.empty()) continue;
    if (nums.size() < 3 || nums.size() > 5) {
      std::ostringstream msg;
      msg << "Error: Error on line " << i_line + 1 << " of file \"" << path << "\"\n"
          << "       Each line should contain either 3-5 numbers, or 0 numbers (blank).\n";
      throw VisfdErr(msg.str());
    }
    std::array<float, 3> c = {{nums[0], nums[1], nums[2]}};
    if (imod_from_one && line_parens)
      for (int k = 0; k < 3; k++) c[k] = std::floor(c[k]) - 1.0f;
    crds.push_back(c);
    float d = nums.size() > 3 ? nums[3] : -1.0f;
    if (d < 0) d = -1.0f;
    diameters.push_back(d * diameter_factor);   // file_io.hpp:470-477: the "no diameter" mark is multiplied too
    scores.push_back(nums.size() > 4 ? nums[4] : score_default);
    i_line++;
  }
  return parens;
}

// Where DiscardOverlappingBlobs runs: the sequential walk on the host below this many blobs, the rounds on the device
// (visfd_hip_discard_overlapping_blobs_ctx) from there on, when a GPU is present; the lists are the same bits either way.
// MEASURED on an MI355X (tools/discard_overlap_time.py, second table of profiles/discard_overlap_time.txt: diameters 8 to 24
// voxels at 10^5 blobs per 512^3, ratio 1, one staged call in a fresh process): the first context costs about 150 ms before
// the device ranks anything, the call itself 6 to 35 ms up to 262 144 blobs; the host walk takes 52.7 ms at 65 536 blobs,
// 177.8 ms at 131 072 (device, all told: 167.5 ms) and 553.6 ms at 262 144 (189.8 ms).  The two meet near 1.25 * 10^5
// blobs; rounded to a power of two.  Without the start-up the device is far ahead (first table: 8.4 ms against 125 ms at
// 10^5 blobs, 204 ms against 19.5 s at 4 * 10^6); the constant does not count on a context that happens to exist.
const double DISCARD_OVERLAP_MIN_BLOBS = 131072.0;   // 2^17

// the context to hand to DiscardOverlappingBlobs for a list of n blobs: null keeps the walk on the host.  The environment
// variable VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS overrides the size (0: always the device) and makes the program say which ran.
visfd_hip_ctx* overlap_context(size_t n) {
  double min_blobs = DISCARD_OVERLAP_MIN_BLOBS;
  const char* e = std::getenv("VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS");
  if (e) min_blobs = std::atof(e);
  visfd_hip_ctx* ctx = nullptr;
  if ((double)n >= min_blobs) {
    try { ctx = hip_detail::context(); } catch (const VisfdErr&) { ctx = nullptr; }   // no GPU: the host walk
  }
  if (e) cerr << "  (discard_overlap: " << (ctx ? "device" : "host") << ")" << std::endl;
  return ctx;
}

// HandleBlobsNonmaxSuppression, bin/filter_mrc/handlers.cpp:421-596 (its supervised tail is in handle_blob_nonmax): the
// lists of the blob files in voxels, filtered by score and size, by the mask (when one is passed) and by overlap
void read_and_filter_blobs(const Run& r, float const* const* const* mask, vector<std::array<float, 3> >& crds,
                           vector<float>& diameters, vector<float>& scores) {
  const Settings& s = r.s;
  const float w = r.vw[0];
  const float inf = std::numeric_limits<float>::infinity();
  for (size_t I = 0; I < s.in_crds_files.size(); I++) {
    vector<std::array<float, 3> > c;
    vector<float> d, sc;
    const bool in_voxels = read_blob_file(s.in_crds_files[I], c, d, sc, s.sphere_decals_foreground, s.sphere_decals_scale);
    if (!in_voxels && w > 0.0f)
      for (size_t i = 0; i < c.size(); i++) {
        for (int k = 0; k < 3; k++) c[i][k] = (float)std::floor((c[i][k] / w) + 0.5);   // handlers.cpp:458
        if (d[i] != -1.0f) d[i] /= w;
      }
    if (s.sphere_decals_diameter >= 0)   // handlers.cpp:474-500: -diameters / -radii replace every diameter of the file
      for (size_t i = 0; i < d.size(); i++) {
        d[i] = s.sphere_decals_diameter;
        if (!s.sphere_decals_diameter_in_voxels && w > 0.0f) d[i] /= w;
      }
    crds.insert(crds.end(), c.begin(), c.end());
    diameters.insert(diameters.end(), d.begin(), d.end());
    scores.insert(scores.end(), sc.begin(), sc.end());
  }
  cerr << " --- discarding blobs in files ---\n\n";
  // handlers.cpp:516-559: any of the four bounds opens the filter; each report line needs BOTH bounds of its pair
  if (s.score_lower != -inf || s.score_upper != inf || s.sphere_diameters_lower != -inf || s.sphere_diameters_upper != inf) {
    if (s.score_lower != -inf && s.score_upper != inf) cerr << "  discarding blobs based on score" << std::endl;
    if (s.sphere_diameters_lower != -inf && s.sphere_diameters_upper != inf)
      cerr << "  discarding blobs based on size (diameter)" << std::endl;
    vector<std::array<float, 3> > c;
    vector<float> d, sc;
    for (size_t i = 0; i < crds.size(); i++)
      if (scores[i] >= s.score_lower && scores[i] <= s.score_upper && diameters[i] >= s.sphere_diameters_lower &&
          diameters[i] <= s.sphere_diameters_upper) {
        c.push_back(crds[i]); d.push_back(diameters[i]); sc.push_back(scores[i]);
      }
    crds.swap(c); diameters.swap(d); scores.swap(sc);
  }
  if (!crds.empty() && mask) {
    cerr << "  discarding blobs outside the mask" << std::endl;
    DiscardMaskedBlobs(crds, diameters, scores, mask, r.size);
  }
  if (s.nonmax_min_radial_separation_ratio > 0 || s.nonmax_max_overlap_large != inf || s.nonmax_max_overlap_small != inf) {
    if (w <= 0.0f)
      throw VisfdErr("Error: Checking for overlapping blobs requires that you either specify the\n"
                     "       voxel width (using the \"-w\" argument).\n");
    cerr << "  discarding overlapping blobs" << std::endl;
    DiscardOverlappingBlobs(overlap_context(crds.size()), crds, diameters, scores, s.nonmax_min_radial_separation_ratio,
                            s.nonmax_max_overlap_large, s.nonmax_max_overlap_small, SORT_DECREASING_MAGNITUDE, &cerr);
  }
  cerr << " " << crds.size() << " blobs remaining" << std::endl;
}

// Which search the supervised tail uses: the walk on the host below this many (training point, blob) pairs, the device
// from there on.  Small lists -- what -discard-blobs usually sees -- then need no GPU at all.
// MEASURED on an MI355X (tools/find_spheres_time.py, second table of profiles/find_spheres_time.txt: 200 training points
// inside blobs, one staged call in a fresh process): the first context costs about 160 ms before the device searches
// anything, the call itself 1 to 34 ms up to 10^7 blobs; the host walk takes 17.9 ms at 2 * 10^7 pairs, 163 ms at 2 * 10^8
// and 868 ms at 2 * 10^9.  The two meet near 2.1 * 10^8 pairs; rounded to a power of two.  The host times include the
// walk's early exit (it goes from the end of the list and stops at the first blob that holds the point), which is what
// training points inside blobs see; points outside every blob are walked against the whole list, 3 to 4 times slower per
// nominal pair, and would cross over at that many fewer pairs.
// The environment variable VISFD_HIP_FIND_SPHERES_MIN_PAIRS overrides it (0: always the device) and makes the program say
// which search ran.
const double FIND_SPHERES_MIN_PAIRS = 268435456.0;   // 2^28

void choose_find_spheres_route(size_t n_training, size_t n_blobs) {
  double min_pairs = FIND_SPHERES_MIN_PAIRS;
  const char* e = std::getenv("VISFD_HIP_FIND_SPHERES_MIN_PAIRS");
  if (e) min_pairs = std::atof(e);
  const bool on_host = (double)n_training * (double)n_blobs < min_pairs;
  FindSpheresOnHost(on_host);
  if (e) cerr << "  (find_spheres: " << (on_host ? "host" : "device") << " search)" << std::endl;
}

void handle_blob_nonmax(Run& r) {
  const Settings& s = r.s;
  const float w = r.vw[0];
  vector<std::array<float, 3> > crds;
  vector<float> diameters, scores;
  read_and_filter_blobs(r, r.mask3d(), crds, diameters, scores);
  // handlers.cpp:598-621: the supervised tail, always after the overlap step.  -auto-thresh without -supervised, or the
  // reverse, does nothing, as in the reference
  if (s.auto_thresh_score && !s.training_pos_crds.empty() && !s.training_neg_crds.empty()) {
    cerr << "  discarding blobs based on score using training data" << std::endl;
    choose_find_spheres_route(s.training_pos_crds.size() + s.training_neg_crds.size(), crds.size());
    DiscardBlobsByScoreSupervised(crds, diameters, scores, s.training_pos_crds, s.training_neg_crds, SORT_DECREASING_MAGNITUDE,
                                  static_cast<float*>(nullptr), static_cast<float*>(nullptr), &cerr);
    cerr << " " << crds.size() << " blobs remaining" << std::endl;
  }
  if (!s.out_crds_file.empty()) {
    const double wp = w > 0.0f ? (double)w : 1.0;
    std::ofstream out(s.out_crds_file.c_str());
    if (!out) throw VisfdErr("Error: unable to open \"" + s.out_crds_file + "\" for writing.\n");
    for (size_t i = 0; i < crds.size(); i++)
      out << crds[i][0] * wp << " " << crds[i][1] * wp << " " << crds[i][2] * wp << " " << diameters[i] * wp << " "
          << scores[i] << std::endl;
  }
}

// HandleBlobScoreSupervisedMulti, bin/filter_mrc/handlers.cpp:648-706: the thresholds that suit several images' blob lists
// and training sets at once; they are only printed
void handle_supervised_multi(Run& r) {
  const Settings& s = r.s;
  const float w = r.vw[0];
  const size_t n_sets = s.multi_in_crds_files.size();
  vector<vector<std::array<float, 3> > > crds(n_sets);
  vector<vector<float> > diameters(n_sets), scores(n_sets);
  size_t pairs_training = 0, pairs_blobs = 0;
  for (size_t I = 0; I < n_sets; I++) {
    read_blob_file(s.multi_in_crds_files[I], crds[I], diameters[I], scores[I], s.sphere_decals_foreground, s.sphere_decals_scale);
    if (s.sphere_decals_diameter >= 0)   // -diameters / -radii: the reader's override (file_io.hpp:474-475)
      for (size_t i = 0; i < diameters[I].size(); i++) diameters[I][i] = s.sphere_decals_diameter;
    if (w > 0.0f)   // handlers.cpp:685-694: every diameter and coordinate, whatever the file's notation
      for (size_t i = 0; i < crds[I].size(); i++) {
        diameters[I][i] /= w;
        for (int k = 0; k < 3; k++) crds[I][i][k] = (float)std::floor((crds[I][i][k] / w) + 0.5);
      }
    pairs_training = std::max(pairs_training, s.multi_training_pos_crds[I].size() + s.multi_training_neg_crds[I].size());
    pairs_blobs = std::max(pairs_blobs, crds[I].size());
  }
  choose_find_spheres_route(pairs_training, pairs_blobs);   // by the largest set
  float lower, upper;
  ChooseBlobScoreThresholdsMulti(crds, diameters, scores, s.multi_training_pos_crds, s.multi_training_neg_crds, &lower, &upper,
                                 SORT_DECREASING_MAGNITUDE, &cerr);
}

// The thickness of one drawn shell (handlers.cpp:751-758 and :957-964): a ratio times the diameter, and where that falls
// below the minimum, 1.0 -- not the minimum; a thickness given in voxels is taken as it is
float shell_thickness_of(const Settings& s, float diameter) {
  float th = s.sphere_decals_shell_thickness;
  if (s.sphere_decals_shell_thickness_is_ratio) {
    th *= diameter;
    if (th < s.sphere_decals_shell_thickness_min) th = 1.0f;
  }
  return th;
}

// HandleDrawSpheres, bin/filter_mrc/handlers.cpp:712-780
void handle_draw_spheres(Run& r) {
  const Settings& s = r.s;
  vector<std::array<float, 3> > crds;
  vector<float> diameters, scores;
  read_and_filter_blobs(r, nullptr, crds, diameters, scores);   // blobs outside the mask are kept
  const size_t n = diameters.size();
  if (!s.sphere_decals_foreground_use_score)
    for (size_t i = 0; i < n; i++) scores[i] = s.sphere_decals_foreground;
  vector<float> th(n);
  for (size_t i = 0; i < n; i++) th[i] = shell_thickness_of(s, diameters[i]);
  std::reverse(crds.begin(), crds.end());
  std::reverse(diameters.begin(), diameters.end());
  std::reverse(th.begin(), th.end());
  std::reverse(scores.begin(), scores.end());
  DrawSpheres(r.size, r.tomo_out.a, r.mask3d(), crds, &diameters, &th, &scores, r.tomo_in.a, s.sphere_decals_background,
              s.sphere_decals_background_scale, s.sphere_decals_background_norm, s.sphere_decals_foreground_norm);
}

// The integer points of the coordinate files of -distance-points / -distance-to-voxels, the handlers' expression
// literally (handlers_unsupported.cpp:1402-1423): a file in voxels has 1 subtracted from every coordinate (on top of what
// the reader did to its lines in parentheses), any other is divided by the voxel width of the axis; then
// floor(c + 0.5), the sum in double.
vector<int32_t> read_integer_points(const Run& r) {
  const Settings& s = r.s;
  vector<int32_t> pts;
  for (size_t I = 0; I < s.in_crds_files.size(); I++) {
    vector<std::array<float, 3> > c;
    vector<float> d, sc;
    const bool in_voxels = read_blob_file(s.in_crds_files[I], c, d, sc, s.sphere_decals_foreground, s.sphere_decals_scale, true);
    for (size_t i = 0; i < c.size(); i++)
      for (int k = 0; k < 3; k++) {
        if (in_voxels) c[i][k] -= 1;
        else c[i][k] /= r.vw[k];
        const double v = std::floor(c[i][k] + 0.5);
        // (the reference converts the double to int whatever its size; beyond int32 the point is farther than any cap)
        pts.push_back(v >= 2147483647.0 ? 2147483647 : v <= -2147483648.0 ? (int32_t)-2147483647 - 1 : (int32_t)v);
      }
  }
  return pts;
}

// HandleDistanceToPoints, handlers_unsupported.cpp:1393-1465: where mask != 0 the output becomes the distance to the
// nearest point, in units of voxel_width[0]
void handle_distance_points(Run& r) {
  const vector<int32_t> pts = read_integer_points(r);
  cerr << " ------ calculating distance to points ------\n" << std::endl;
  hip_detail::check(visfd_hip_distance_to_points(hip_detail::context(), r.tomo_out.data(), r.mask_flat(), r.size[0], r.size[1],
                                                 r.size[2], pts.data(), (int64_t)(pts.size() / 3), r.vw[0]));
}

// HandleDistancePointsToFeature, handlers_unsupported.cpp:1470-1550: one line per point, the distance to the nearest voxel
// inside the mask whose brightness lies in [A, B]; the image is left as it is
void handle_distance_to_voxels(Run& r) {
  const Settings& s = r.s;
  const vector<int32_t> pts = read_integer_points(r);
  cerr << " ------ calculating distance from points to feature ------\n" << std::endl;
  vector<float> dist(pts.size() / 3);
  hip_detail::check(visfd_hip_distance_from_points(hip_detail::context(), r.tomo_in.data(), r.mask_flat(), r.size[0], r.size[1],
                                                   r.size[2], s.out_thresh_a_value, s.out_thresh_b_value, pts.data(),
                                                   (int64_t)dist.size(), r.vw[0], dist.data()));
  std::fstream out;
  out.open(s.out_distances_file.c_str(), std::ios::out);
  if (!out) throw VisfdErr("Error: unable to open \"" + s.out_distances_file + "\" for writing.\n");
  for (size_t i = 0; i < dist.size(); i++) out << dist[i] << std::endl;
}

// HandleBinning, bin/filter_mrc/handlers.cpp:2361-2425: the image (and the mask) shrink by `bin` per axis
// (BinArray3D averages; trailing voxels are dropped) and the voxel width grows by the same factor.
void bin_image(Mrc& img, int bin, double voxel_width_binned) {
  int ssz[3] = {img.nx, img.ny, img.nz};
  int dsz[3] = {img.nx / bin, img.ny / bin, img.nz / bin};
  if (dsz[0] < 1 || dsz[1] < 1 || dsz[2] < 1) throw VisfdErr("Error: the image is too small for this bin size.\n");
  Mrc tmp;
  tmp.alloc(dsz[0], dsz[1], dsz[2]);
  BinArray3D(ssz, dsz, img.a, tmp.a);
  std::memcpy(tmp.raw_header, img.raw_header, 1024);
  tmp.mode = img.mode;
  tmp.loaded = true;
  for (int d = 0; d < 3; d++) tmp.cella[d] = (float)(voxel_width_binned * dsz[d]);
  img.swap(tmp);
}

// the tail of HandleTV (handlers.cpp:2315-2355): an image that was binned WITHOUT the user asking for it
// goes back to the original size (nearest-lower sampling)
void unbin_image(Mrc& img, const int size_orig[3], const float cella_orig[3]) {
  int ssz[3] = {img.nx, img.ny, img.nz};
  Mrc big;
  big.alloc(size_orig[0], size_orig[1], size_orig[2]);
  UnbinArray3D(ssz, size_orig, img.a, big.a);
  std::memcpy(big.raw_header, img.raw_header, 1024);
  big.mode = img.mode;
  big.loaded = true;
  for (int d = 0; d < 3; d++) big.cella[d] = cella_orig[d];
  img.swap(big);
}

float ratio_of(const Settings& s) {
  return s.truncate_ratio > 0 ? s.truncate_ratio : visfd_hip_ratio_from_threshold(s.truncate_threshold);
}

// One rank's slab handle for `-slab RANK WORLD IDFILE`: rank 0 makes the RCCL id and publishes it as IDFILE (written under a
// temporary name, then renamed; removed again once every rank has joined); the other ranks wait for the file.  IDFILE "-"
// with WORLD 1 runs without a communicator.
visfd_hip_slab* open_slab(const Settings& s, int64_t nz, int ghost) {
  visfd_hip_ctx* ctx = hip_detail::context();
  unsigned char id[128];
  const bool with_id = !(s.slab_id_file == "-" && s.slab_world == 1);
  if (s.slab_id_file == "-" && s.slab_world > 1) throw VisfdErr("Error: -slab with more than one rank needs an id file.\n");
  if (with_id) {
    if (s.slab_rank == 0) {
      std::remove(s.slab_id_file.c_str());   // an id file left behind by an earlier run must not be picked up by this run's ranks
      hip_detail::check(visfd_hip_slab_unique_id(id));
      const string tmp = s.slab_id_file + ".tmp";
      { std::ofstream f(tmp.c_str(), std::ios::binary); f.write(reinterpret_cast<const char*>(id), 128);
        if (!f) throw VisfdErr("Error: unable to write \"" + tmp + "\".\n"); }
      if (std::rename(tmp.c_str(), s.slab_id_file.c_str()) != 0) throw VisfdErr("Error: unable to create \"" + s.slab_id_file + "\".\n");
    } else {
      // IDFILE must be unique per run.  Rank 0 removes it before it publishes a new id and again once the communicator is
      // up; a file older than the ten minutes a rank waits is taken to be a leftover and ignored.
      const std::time_t started = std::time(nullptr);
      bool got = false;
      for (int tries = 0; tries < 12000 && !got; tries++) {   // up to 10 minutes
        struct stat st;
        const bool fresh = ::stat(s.slab_id_file.c_str(), &st) == 0 && st.st_mtime + 600 >= started;
        std::ifstream f(s.slab_id_file.c_str(), std::ios::binary);
        if (fresh && f && f.read(reinterpret_cast<char*>(id), 128) && f.gcount() == 128) got = true;
        else std::this_thread::sleep_for(std::chrono::milliseconds(50));
      }
      if (!got) throw VisfdErr("Error: the id file \"" + s.slab_id_file + "\" did not appear (is rank 0 running?).\n");
    }
  }
  visfd_hip_slab* slab = nullptr;
  hip_detail::check(visfd_hip_slab_create_rccl(ctx, with_id ? id : nullptr, s.slab_rank, s.slab_world, nz, ghost, &slab));
  if (with_id && s.slab_rank == 0) std::remove(s.slab_id_file.c_str());   // every rank has joined: the id has served
  return slab;
}

// this rank's planes as an MRC file of their own: the input's header with nz, the cell's z extent and the z origin of the slab
void write_slab_part(const Settings& s, Mrc& tomo_in, Mrc& part, int64_t z0) {
  part.copy_header_from(tomo_in);
  float fw[256];
  std::memcpy(fw, part.raw_header, 1024);
  const float dz = tomo_in.cella[2] / (float)tomo_in.nz;
  part.cella[2] = dz * (float)part.nz;
  fw[51] += dz * (float)z0;                                // MRC2014 origin z (word 52)
  std::memcpy(part.raw_header, fw, 1024);
  if (!s.out.empty()) {
    cerr << "writing this slab's planes (in 32-bit float mode)\n";
    part.write(s.out, part);
  }
}

// -gauss ... -slab: this rank filters its owned planes (the ghost planes come from the neighbours; the normaliser follows
// global plane indices, so only the true faces of the volume are borders) and writes them.
void gauss_slab(Run& r) {
  const Settings& s = r.s;
  Mrc& tomo_in = r.tomo_in;
  Mrc out;
  if (!s.mask.empty()) throw VisfdErr("Error: -slab does not combine with -mask.\n");
  int hw[3];
  hip_detail::check(visfd_hip_gauss_halfwidths(s.width_a, r.ratio, hw));
  visfd_hip_slab* slab = open_slab(s, tomo_in.nz, hw[2]);
  int64_t lay[7];
  hip_detail::check(visfd_hip_slab_layout(slab, lay));
  const int64_t z0 = lay[0], z1 = lay[1];
  cerr << "slab " << s.slab_rank << " of " << s.slab_world << ": planes [" << z0 << ", " << z1 << "), ghost depth " << hw[2] << "\n";
  out.alloc(tomo_in.nx, tomo_in.ny, (int)(z1 - z0));
  const size_t plane = (size_t)tomo_in.nx * tomo_in.ny;
  float A = 0;
  const int rc = visfd_hip_apply_gauss_slab(slab, tomo_in.data() + (size_t)z0 * plane, tomo_in.nx, tomo_in.ny, s.width_a, hw,
                                            s.normalize ? 1 : 0, out.data(), &A);
  visfd_hip_slab_destroy(slab);
  hip_detail::check(rc);
  cerr << "  ... where  A = " << A << "\n";
  write_slab_part(s, tomo_in, out, z0);
}

// -blob ... -slab: the blobs of this rank's owned planes (absolute score thresholds only: ratios need the global best score).
// Rows come back with GLOBAL z; every rank writes its own list files, tools/join_slabs.py merges them.
void blob_slab(Run& r, vector<visfd_hip_blob>* mins, vector<visfd_hip_blob>* maxs) {
  const Settings& s = r.s;
  Mrc& tomo_in = r.tomo_in;
  const float ratio = r.ratio;
  if (!s.mask.empty()) throw VisfdErr("Error: -slab does not combine with -mask.\n");
  for (int d = 0; d < 3; d++)
    if (s.blob_aspect_ratio[d] != 1.0f) throw VisfdErr("Error: -slab runs isotropic blob detection only (no -blob-aspect-ratio).\n");
  vector<float> sig(s.blob_diameters.size());
  hip_detail::check(visfd_hip_blob_diameters_to_sigmas(s.blob_diameters.data(), (int)sig.size(), sig.data()));
  int ghost = 0;
  hip_detail::check(visfd_hip_blob_halo_depth(sig.data(), (int)sig.size(), s.delta, ratio, &ghost));
  visfd_hip_slab* slab = open_slab(s, tomo_in.nz, ghost);
  int64_t lay[7];
  hip_detail::check(visfd_hip_slab_layout(slab, lay));
  const int64_t z0 = lay[0];
  cerr << "slab " << s.slab_rank << " of " << s.slab_world << ": planes [" << z0 << ", " << lay[1] << "), ghost depth " << ghost << "\n";
  const size_t plane = (size_t)tomo_in.nx * tomo_in.ny;
  int64_t cap = 1 << 16, nmin = 0, nmax = 0;
  int rc;
  for (;;) {
    mins->resize((size_t)cap);
    maxs->resize((size_t)cap);
    rc = visfd_hip_blob_dog_slab(slab, tomo_in.data() + (size_t)z0 * plane, tomo_in.nx, tomo_in.ny, sig.data(), (int)sig.size(), s.delta,
                                 ratio, s.score_upper, s.score_lower, mins->data(), cap, &nmin, maxs->data(), cap, &nmax);
    if (rc != VISFD_HIP_ECAPACITY) break;
    cap = std::max(std::max(nmin, nmax), cap) + 16;
  }
  visfd_hip_slab_destroy(slab);
  hip_detail::check(rc);
  mins->resize((size_t)nmin);
  maxs->resize((size_t)nmax);
}

// -membrane ... -tv ... -slab: this rank's planes of the voted saliency (halos, the global top-fraction threshold and the
// overlapped votes are csrc/slab.hip's business), written to this rank's own -out file; tools/join_slabs.py stacks the files.
void membrane_slab(Run& r, int order) {
  const Settings& s = r.s;
  Mrc& tomo_in = r.tomo_in;
  const float ratio = r.ratio;
  Mrc out;
  if (!(s.tv_sigma > 0)) throw VisfdErr("Error: -slab needs -tv (tensor voting).\n");
  if (!s.hessian_thr_is_fraction) throw VisfdErr("Error: -slab needs the fractional threshold (-tv-best), not -detection-threshold.\n");
  if (!s.mask.empty() || !s.load_base.empty() || !s.save_base.empty() || s.cluster_connected_voxels)
    throw VisfdErr("Error: -slab runs the plain -membrane ... -tv stage only (no -mask, -save/-load-progress, -connect).\n");
  int h_tv = 0;
  hip_detail::check(visfd_hip_tv_tables(s.tv_sigma, s.tv_truncate, &h_tv, nullptr, nullptr));
  const float sigma_bg = s.width_b[0] > 0.0f ? s.width_b[0] : 0.0f;
  const int ghost = std::max(std::max(h_tv, (int)std::floor(s.width_a[0] * ratio) + 1), (int)std::floor(sigma_bg * ratio));
  visfd_hip_slab* slab = open_slab(s, tomo_in.nz, ghost);
  int64_t lay[7];
  hip_detail::check(visfd_hip_slab_layout(slab, lay));
  const int64_t z0 = lay[0], z1 = lay[1];
  cerr << "slab " << s.slab_rank << " of " << s.slab_world << ": planes [" << z0 << ", " << z1 << "), ghost depth " << ghost << "\n";
  out.alloc(tomo_in.nx, tomo_in.ny, (int)(z1 - z0));
  float thr = 0;
  const size_t plane = (size_t)tomo_in.nx * tomo_in.ny;
  const int rc = visfd_hip_membrane_detect_slab_bg(slab, tomo_in.data() + (size_t)z0 * plane, tomo_in.nx, tomo_in.ny, s.width_a[0], ratio,
                                                   order, s.hessian_thr, s.tv_sigma, s.tv_exponent, s.tv_truncate, sigma_bg,
                                                   s.normalize ? 1 : 0, out.data(), nullptr, &thr);
  visfd_hip_slab_destroy(slab);
  hip_detail::check(rc);
  cerr << "  (saliency threshold = " << thr << ")\n";
  write_slab_part(s, tomo_in, out, z0);
}

// the input and the mask, of one size
void load(Run& r) {
  const Settings& s = r.s;
  r.tomo_in.read(s.in);
  if (!s.mask.empty()) {
    r.mask.read(s.mask);
    if (r.mask.nx != r.tomo_in.nx || r.mask.ny != r.tomo_in.ny || r.mask.nz != r.tomo_in.nz)
      throw VisfdErr("Error: The size of the mask image does not match the size of the input image.\n");
    if (s.use_mask_select) {   // filter_mrc.cpp:100-107: the voxels of one label become the mask
      float* mp = r.mask.data();
      for (size_t i = 0; i < r.mask.nvox(); i++) mp[i] = (mp[i] == s.mask_select) ? 1.0f : 0.0f;
    }
  }
  r.size[0] = r.tomo_in.nx; r.size[1] = r.tomo_in.ny; r.size[2] = r.tomo_in.nz;
  for (int d = 0; d < 3; d++) { r.size_orig[d] = r.size[d]; r.cella_orig[d] = r.tomo_in.cella[d]; }
}

// -mask-rect, -mask-sphere and their -subtract forms (filter_mrc.cpp:220-286): drawn into the mask, which starts as zeros
// when no file was given
void draw_mask_regions(Run& r, Settings& s) {
  if (!r.mask.loaded) {
    r.mask.alloc(r.size[0], r.size[1], r.size[2]);
    std::memset(r.mask.data(), 0, r.mask.nvox() * 4);
    r.mask.copy_header_from(r.tomo_in);
    r.mask.loaded = true;
  }
  const float scale = (float)(1.0 / r.bin);   // always voxels (see -mask-crds-units): only binning rescales them
  for (size_t k = 0; k < s.mask_regions.size(); k++) {
    SimpleRegion<float>& g = s.mask_regions[k];
    if (g.type == SimpleRegion<float>::RECT) {
      g.data.rect.xmin *= scale; g.data.rect.xmax *= scale; g.data.rect.ymin *= scale;
      g.data.rect.ymax *= scale; g.data.rect.zmin *= scale; g.data.rect.zmax *= scale;
    } else {
      g.data.sphere.r *= scale; g.data.sphere.x0 *= scale; g.data.sphere.y0 *= scale; g.data.sphere.z0 *= scale;
    }
  }
  DrawRegions(r.size, r.mask.a, static_cast<const float* const* const*>(nullptr), s.mask_regions, true);
}

// From the files to what the handlers work on, in the reference's order: voxel width, binning, lengths in voxels (`s` is
// the Settings that r.s refers to), the mask regions, the output as a copy of the input
void prepare(Run& r, Settings& s) {
  if (s.voxel_width > 0) r.vw[0] = r.vw[1] = r.vw[2] = s.voxel_width;
  else {
    r.vw[0] = r.tomo_in.cella[0] / r.size[0];  // handlers.cpp:2429-2475: inferred from the header
    r.vw[1] = r.vw[2] = r.vw[0];
    if (!(r.vw[0] > 0)) r.vw[0] = r.vw[1] = r.vw[2] = 1.0f;
  }
  // ---- binning (filter_mrc.cpp:118-209): explicit (-bin N) or automatic for wide features ----
  r.bin = s.bin;
  if (r.bin == 0) {
    r.bin = 1;
    if (s.tv_sigma > 0 && s.width_a[0] > 1.8 * r.vw[0])
      r.bin = (int)std::ceil(s.width_a[0] / (1.8 * r.vw[0]));
    else if (!(s.tv_sigma > 0) && !s.blob_diameters.empty() && s.blob_diameters[0] > 15.0 * r.vw[0])
      r.bin = (int)std::ceil(s.blob_diameters[0] / (15.0 * r.vw[0]));
    if (r.bin > 1)
      cerr << "--- WARNING: this would be very slow unless binning is used.\n"
              "--- BINNING THE IMAGE BY A FACTOR OF " << r.bin << "\n"
              "---           To prevent this, use the \"-bin 1\" argument.\n";
  }
  if (r.bin > 1) {
    const double w0 = s.voxel_width > 0 ? (double)s.voxel_width : (double)(r.tomo_in.cella[0] / r.tomo_in.nx);
    const double wb = w0 * r.bin;                      // handlers.cpp:2372-2385
    bin_image(r.tomo_in, r.bin, wb);
    if (r.mask.loaded) bin_image(r.mask, r.bin, wb);
    r.size[0] = r.tomo_in.nx; r.size[1] = r.tomo_in.ny; r.size[2] = r.tomo_in.nz;
    if (s.voxel_width > 0) r.vw[0] = r.vw[1] = r.vw[2] = s.voxel_width * r.bin;           // handlers.cpp:2445-2460
    else for (int d = 0; d < 3; d++) r.vw[d] = r.tomo_in.cella[d] / r.size[d];
  }
  cerr << "voxel width = " << r.vw[0] << "\n";
  for (size_t k = 0; k < s.must_link_crds.size(); k++)      // filter_mrc.cpp:372-379: physical units -> voxels, or
    s.must_link_crds[k] /= s.must_link_in_voxels ? (float)r.bin : r.vw[k % 3];   // voxels of the unbinned image -> binned
  // filter_mrc.cpp:340-352: the -supervised points likewise.  The multi sets' loops of the reference (:354-370) are bounded
  // by the sizes of THESE lists, which are empty whenever multi sets exist (settings.hpp refuses the combination): the
  // multi coordinates stay as read
  for (size_t i = 0; i < s.training_pos_crds.size(); i++)
    for (int d = 0; d < 3; d++) s.training_pos_crds[i][d] /= s.is_training_pos_in_voxels ? (float)r.bin : r.vw[d];
  for (size_t i = 0; i < s.training_neg_crds.size(); i++)
    for (int d = 0; d < 3; d++) s.training_neg_crds[i][d] /= s.is_training_neg_in_voxels ? (float)r.bin : r.vw[d];
  for (int d = 0; d < 3; d++) { s.width_a[d] /= r.vw[d]; s.width_b[d] /= r.vw[d]; s.log_width[d] /= r.vw[d]; s.template_background_radius[d] /= r.vw[d]; }
  s.tv_sigma /= r.vw[0];
  for (size_t k = 0; k < s.blob_diameters.size(); k++) s.blob_diameters[k] /= r.vw[0];
  s.morph_r /= r.vw[0];      // filter_mrc.cpp:297-298 (bmax is not a length)
  s.morph_rmax /= r.vw[0];
  if (!s.sphere_decals_shell_thickness_is_ratio) s.sphere_decals_shell_thickness /= r.vw[0];   // filter_mrc.cpp:333-336
  else s.sphere_decals_shell_thickness /= r.bin;
  if (!s.mask_regions.empty()) draw_mask_regions(r, s);
  r.tomo_out.alloc(r.size[0], r.size[1], r.size[2]);
  std::memcpy(r.tomo_out.data(), r.tomo_in.data(), r.tomo_in.nvox() * 4);   // filter_mrc.cpp:398
  r.ratio = ratio_of(s);
  if (s.slab_world > 0 && r.bin > 1) throw VisfdErr("Error: -slab does not combine with binning (use -bin 1).\n");
  if (s.slab_world > 0 && s.type != Settings::GAUSS && s.type != Settings::BLOB && s.type != Settings::SURFACE_RIDGE)
    throw VisfdErr("Error: -slab runs with -gauss, -blob and -membrane ... -tv.\n");
}

// The handlers: one per Settings type.  handle_gauss and handle_membrane return false after a -slab run, which has written
// this rank's planes itself and ends without finish().
bool handle_gauss(Run& r) {
  const Settings& s = r.s;
  if (s.slab_world > 0) {
    cerr << "filter_type = Gaussian (Z-slab mode)\n";
    gauss_slab(r);
    return false;
  }
  cerr << "filter_type = Gaussian\n";
  const float A = ApplyGauss(r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.width_a, s.truncate_ratio, s.truncate_threshold,
                             s.normalize, &cerr);
  cerr << " Filter Used: A discrete Gaussian kernel, approximately equal to\n"
          " h(x,y,z)   ≈ A*exp(-0.5*((x/σ_x)^2 + (y/σ_y)^2 + (z/σ_z)^2))\n"
          " ... where  A = " << A << "\n";
  return true;
}

// HandleLocalFluctuations, handlers.cpp:1254-1271
void handle_fluctuations(Run& r) {
  const Settings& s = r.s;
  LocalFluctuationsByRadius(r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.template_background_radius,
                            s.template_background_exponent, s.truncate_ratio, s.truncate_threshold, s.normalize, &cerr);
}

// HandleGGauss, handlers.cpp:167-213
void handle_ggauss(Run& r) {
  const Settings& s = r.s;
  int hw[3];
  float A = 0;
  hip_detail::check(visfd_hip_gengauss3d_halfwidths(s.width_a, s.m_exp, s.truncate_ratio, s.truncate_threshold, hw));
  hip_detail::check(visfd_hip_apply_ggauss(hip_detail::context(), r.tomo_in.data(), r.tomo_out.data(),
                                           r.mask_flat(), r.size[0], r.size[1], r.size[2], s.width_a,
                                           s.m_exp, hw, s.normalize ? 1 : 0, &A));
  cerr << " Filter Used:\n"
          " h(x,y,z)   = A*exp(-((x/a_x)^2 + (y/a_y)^2 + (z/a_z)^2)^(m/2))\n"
          "  ... where      A = " << A << "\n"
          "                 m = " << s.m_exp << "\n"
          "   (a_x, a_y, a_z) = " << "(" << s.width_a[0] << " " << s.width_a[1] << " " << s.width_a[2] << ")\n";
  cerr << " You can plot a slice of this function\n"
       << "     in the X direction using:\n"
          " draw_filter_1D.py -ggauss " << A << " " << s.width_a[0] << " " << s.m_exp << std::endl;
  if (s.width_a[1] != s.width_a[0] || s.width_a[2] != s.width_a[0]) {
    cerr << " and in the Y direction using:\n"
            " draw_filter_1D.py -ggauss " << A << " " << s.width_a[1] << " " << s.m_exp << std::endl;
    cerr << " and in the Z direction using:\n"
            " draw_filter_1D.py -ggauss " << A << " " << s.width_a[2] << " " << s.m_exp << std::endl;
  }
}

// HandleDogg, handlers.cpp:265-293; the report is _GenFilterDogg3D's, filter3d_variants.hpp:347-379
void handle_dogg(Run& r) {
  const Settings& s = r.s;
  cerr << "filter_type = Difference-of-Generalized-Gaussians (DOGG)\n";
  if (r.mask.loaded)
    cerr << "WARNING: -dogg with -mask: the reference program crashes at the first voxel outside the mask\n"
            "         (it applies the filter with a mask and without a denominator).  This program writes 0 there.\n";
  float A = 0, B = 0;
  hip_detail::check(visfd_hip_apply_dogg(hip_detail::context(), r.tomo_in.data(), r.tomo_out.data(),
                                         r.mask_flat(), r.size[0], r.size[1], r.size[2], s.width_a,
                                         s.width_b, s.m_exp, s.n_exp, s.truncate_ratio, s.truncate_threshold, &A, &B));
  cerr << "\n"
          " Filter Used:\n"
          " h(x,y,z)   = h_a(x,y,z) - h_b(x,y,z)\n"
          " h_a(x,y,z) = A*exp(-((x/a_x)^2 + (y/a_y)^2 + (z/a_z)^2)^(m/2))\n"
          " h_b(x,y,z) = B*exp(-((x/b_x)^2 + (y/b_y)^2 + (z/b_z)^2)^(n/2))\n"
          "  ... where      A = " << A << "\n"
          "                 B = " << B << "\n"
          "                 m = " << s.m_exp << "\n"
          "                 n = " << s.n_exp << "\n"
          "   (a_x, a_y, a_z) = " << "(" << s.width_a[0] << " " << s.width_a[1] << " " << s.width_a[2] << ")\n"
          "   (b_x, b_y, b_z) = " << "(" << s.width_b[0] << " " << s.width_b[1] << " " << s.width_b[2] << ")\n";
  cerr << " You can plot a slice of this function\n"
       << "     in the X direction using:\n"
          " draw_filter_1D.py -dogg " << A << " " << B << " " << s.width_a[0] << " " << s.width_b[0] << " " << s.m_exp
       << " " << s.n_exp << std::endl;
  if (s.width_a[1] != s.width_a[0] || s.width_a[2] != s.width_a[0]) {
    cerr << " and in the Y direction using:\n"
            " draw_filter_1D.py -dogg " << A << " " << B << " " << s.width_a[1] << " " << s.width_b[1] << " " << s.m_exp
         << " " << s.n_exp << std::endl;
    cerr << " and in the Z direction using:\n"
            " draw_filter_1D.py -dogg " << A << " " << B << " " << s.width_a[2] << " " << s.width_b[2] << " " << s.m_exp
         << " " << s.n_exp << std::endl;
  }
}

void handle_dog(Run& r) {
  const Settings& s = r.s;
  cerr << "filter_type = Difference of Gaussians (DoG)\n";
  // bin/filter_mrc/filter3d_variants.hpp:542-597: each Gaussian has its own window
  Mrc tmp;
  tmp.alloc(r.size[0], r.size[1], r.size[2]);
  const float A = ApplyGauss(r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.width_a, s.truncate_ratio, s.truncate_threshold, true);
  const float B = ApplyGauss(r.size, r.tomo_in.a, tmp.a, r.mask3d(), s.width_b, s.truncate_ratio, s.truncate_threshold, true);
  float* o = r.tomo_out.data();
  const float* t = tmp.data();
  for (size_t i = 0; i < r.tomo_out.nvox(); i++) o[i] -= t[i];
  cerr << "  ... where      A = " << A << "\n                 B = " << B << "\n";
}

void handle_log(Run& r) {
  const Settings& s = r.s;
  cerr << "filter_type = Laplacian of Gaussians (LoG)\n";
  float A = 0, B = 0;
  ApplyLog(r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.log_width, s.delta, r.ratio, &A, &B, &cerr);
  cerr << "  ... where      A = " << A << "\n                 B = " << B << "\n";
}

// the blobs of one run, minima [0] and maxima [1]: voxel coordinates, diameters in voxels, scores
struct Blobs {
  vector<std::array<float, 3> > c[2];
  vector<float> d[2], sc[2];
};

// detection, plain or of this rank's planes (-slab: global z).  Returns what -slab with more than one rank appends to the
// names of the list files: every rank writes "<file>.slab<RANK>" (tools/join_slabs.py)
string detect_blobs(Run& r, Blobs& b) {
  const Settings& s = r.s;
  if (s.slab_world == 0) {
    BlobDogD(r.size, r.tomo_in.a, r.mask3d(), s.blob_diameters, &b.c[0], &b.c[1], &b.d[0], &b.d[1], &b.sc[0], &b.sc[1],
             s.blob_aspect_ratio, s.delta, r.ratio, s.score_upper, s.score_lower, s.score_bounds_are_ratios, &cerr);
    return string();
  }
  vector<visfd_hip_blob> bl[2];
  blob_slab(r, &bl[0], &bl[1]);
  for (int side = 0; side < 2; side++) {
    vector<std::array<float, 3> >& c = b.c[side];
    vector<float>& dia = b.d[side];
    vector<float>& sc = b.sc[side];
    vector<float> sg(bl[side].size());
    c.resize(sg.size()); dia.resize(sg.size()); sc.resize(sg.size());
    for (size_t i = 0; i < sg.size(); i++) {
      c[i][0] = (float)bl[side][i].ix; c[i][1] = (float)bl[side][i].iy; c[i][2] = (float)bl[side][i].iz;
      sg[i] = bl[side][i].sigma; sc[i] = bl[side][i].score;
    }
    if (!sg.empty()) hip_detail::check(visfd_hip_blob_sigmas_to_diameters(sg.data(), (int)sg.size(), dia.data()));
  }
  std::ostringstream o;
  if (s.slab_world > 1) o << ".slab" << s.slab_rank;
  return o.str();
}

// physical units + sort by score (handlers.cpp:853-909), ties keep list order.  draw_d and draw_s are what the picture is
// drawn from: physical diameters and scores, sorted where a file is written
void write_blob_lists(Run& r, const Blobs& b, const string& slab_suffix, vector<float> draw_d[2], vector<float> draw_s[2]) {
  const Settings& s = r.s;
  for (int side = 0; side < 2; side++) {
    const string fname = (side ? s.blob_max_file : s.blob_min_file).empty() ? string() : (side ? s.blob_max_file : s.blob_min_file) + slab_suffix;
    const vector<std::array<float, 3> >& c = b.c[side];
    const vector<float>& dia = b.d[side];
    const vector<float>& sc = b.sc[side];
    vector<size_t> idx(c.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
    if (!fname.empty())
      std::stable_sort(idx.begin(), idx.end(), [&](size_t p, size_t q) { return side ? sc[p] > sc[q] : sc[p] < sc[q]; });
    for (size_t k = 0; k < idx.size(); k++) {
      draw_d[side].push_back(dia[idx[k]] * r.vw[0]);
      draw_s[side].push_back(sc[idx[k]]);
    }
    if (fname.empty()) continue;
    std::ofstream out(fname.c_str());
    if (!out) throw VisfdErr("Error: unable to open \"" + fname + "\" for writing.\n");
    for (size_t k = 0; k < idx.size(); k++) {
      const size_t i = idx[k];
      out << c[i][0] * r.vw[0] << " " << c[i][1] * r.vw[1] << " " << c[i][2] * r.vw[2] << " " << dia[i] * r.vw[0] << " "
          << sc[i] << "\n";
    }
  }
}

// handlers.cpp:933-978: every blob as a shell over the input image, minima first, then maxima reversed.  The
// reference sorts the diameters and scores it writes to a file and leaves the voxel coordinates in detection
// order, then draws from both: so does this.
void draw_blobs(Run& r, const Blobs& b, const vector<float> draw_d[2], const vector<float> draw_s[2]) {
  const Settings& s = r.s;
  vector<std::array<float, 3> > crds(b.c[0]);
  crds.insert(crds.end(), b.c[1].rbegin(), b.c[1].rend());
  vector<float> dia(draw_d[0]), sc(draw_s[0]);
  dia.insert(dia.end(), draw_d[1].rbegin(), draw_d[1].rend());
  sc.insert(sc.end(), draw_s[1].rbegin(), draw_s[1].rend());
  vector<float> th(crds.size());
  for (size_t i = 0; i < crds.size(); i++) {
    dia[i] = dia[i] / r.vw[0];
    th[i] = s.sphere_decals_shell_thickness;
    if (s.sphere_decals_shell_thickness_is_ratio) th[i] *= dia[i];
    dia[i] *= s.sphere_decals_scale;
    if (th[i] < s.sphere_decals_shell_thickness_min) th[i] = 1.0f;
  }
  DrawSpheres(r.size, r.tomo_out.a, r.mask3d(), crds, &dia, &th, &sc, r.tomo_in.a, s.sphere_decals_background,
              s.sphere_decals_background_scale, s.sphere_decals_background_norm, false);
}

void handle_blob(Run& r) {
  Blobs b;
  vector<float> draw_d[2], draw_s[2];
  const string slab_suffix = detect_blobs(r, b);
  write_blob_lists(r, b, slab_suffix, draw_d, draw_s);
  if (!r.s.out.empty()) draw_blobs(r, b, draw_d, draw_s);
}

// HandleDilation ... HandleTopHatBlack, handlers.cpp:41-145: tomo_out starts as a copy of the input (the top-hats read it)
void handle_morphology(Run& r) {
  const Settings& s = r.s;
  switch (s.morph_op) {
    case VISFD_HIP_MORPH_DILATE:
      DilateSphere(s.morph_r, r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.morph_rmax, s.morph_bmax, &cerr); break;
    case VISFD_HIP_MORPH_ERODE:
      ErodeSphere(s.morph_r, r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.morph_rmax, s.morph_bmax, &cerr); break;
    case VISFD_HIP_MORPH_OPEN:
      OpenSphere(s.morph_r, r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.morph_rmax, s.morph_bmax, &cerr); break;
    case VISFD_HIP_MORPH_CLOSE:
      CloseSphere(s.morph_r, r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.morph_rmax, s.morph_bmax, &cerr); break;
    case VISFD_HIP_MORPH_TOP_HAT_WHITE:
      WhiteTopHatSphere(s.morph_r, r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.morph_rmax, s.morph_bmax, &cerr); break;
    default:
      BlackTopHatSphere(s.morph_r, r.size, r.tomo_in.a, r.tomo_out.a, r.mask3d(), s.morph_rmax, s.morph_bmax, &cerr); break;
  }
}

// HandleExtrema, handlers.cpp:1086-1245
void handle_extrema(Run& r) {
  const Settings& s = r.s;
  std::memset(r.tomo_out.data(), 0, r.tomo_out.nvox() * 4);
  vector<std::array<float, 3> > crds[2];
  vector<float> scores[2];
  vector<size_t> nvoxels[2];
  const size_t num_extrema =
      _FindExtrema(r.size, r.tomo_in.a, r.mask3d(), s.find_minima ? &crds[0] : nullptr, s.find_maxima ? &crds[1] : nullptr,
                   s.find_minima ? &scores[0] : nullptr, s.find_maxima ? &scores[1] : nullptr,
                   s.find_minima ? &nvoxels[0] : nullptr, s.find_maxima ? &nvoxels[1] : nullptr, s.score_upper,
                   s.score_lower, s.neighbor_connectivity, s.extrema_on_boundary, r.tomo_out.a, &cerr);
  cerr << "Found " << num_extrema << " extrema" << std::endl;
  // handlers.cpp:1165-1211: extrema closer than a diameter (as given: it is not divided by the voxel width) times the
  // separation ratio are thinned, the better score staying.  The voxel counts are not thinned with them: entry k of
  // the thinned list is written with count k of the full one, as in the reference.
  if (s.sphere_decals_diameter > 0 && s.nonmax_min_radial_separation_ratio > 0.0f)
    for (int side = 0; side < 2; side++) {
      vector<float> diam(crds[side].size(), s.sphere_decals_diameter * s.nonmax_min_radial_separation_ratio);
      if (!crds[side].empty() && r.mask3d()) DiscardMaskedBlobs(crds[side], diam, scores[side], r.mask3d(), r.size);
      DiscardOverlappingBlobs(overlap_context(crds[side].size()), crds[side], diam, scores[side], s.nonmax_min_radial_separation_ratio,
                              s.nonmax_max_overlap_large, s.nonmax_max_overlap_small,
                              side ? SORT_DECREASING : SORT_INCREASING, &cerr);
    }
  for (int side = 0; side < 2; side++) {
    const string& fname = side ? s.find_maxima_file : s.find_minima_file;
    if (crds[side].empty() || !(side ? s.find_maxima : s.find_minima)) continue;   // no file for an empty list
    std::fstream out;
    out.open(fname.c_str(), std::ios::out);
    // "for reading" is the reference's wording for this file it writes (handlers.cpp:1223, :1236)
    if (!out) throw VisfdErr("Error: unable to open \"" + fname + "\" for reading.\n");
    for (size_t k = 0; k < crds[side].size(); k++)
      out << crds[side][k][0] * r.vw[0] << " " << crds[side][k][1] * r.vw[1] << " " << crds[side][k][2] * r.vw[2] << " "
          << nvoxels[side][k] << " " << scores[side][k] << "\n";
  }
}

// labels as a float image: -1 (undefined) becomes the largest label plus one, or the -undefined-out value.  The caller
// finds the largest label: the watershed over every voxel, the clustering over the unmasked ones.
template <class Label>
void labels_to_image(const Settings& s, const Label* lab, Label max_label, float* o, size_t n) {
  for (size_t i = 0; i < n; i++) {
    o[i] = (float)lab[i];
    if (lab[i] == -1) o[i] = s.undefined_voxels_are_max ? (float)(max_label + 1) : s.undefined_voxel_brightness;
  }
}

// a 3-D table that lives as long as its holder; null until alloc()
template <class T>
struct Table3D {
  T*** a = nullptr;
  Table3D() {}
  Table3D(const Table3D&) = delete;
  Table3D& operator=(const Table3D&) = delete;
  ~Table3D() { Dealloc3D(a); }
  void alloc(const int size[3]) { a = Alloc3D<T>(size); }
};

// HandleWatershed, handlers.cpp:1280-1391: Watershed is called with label_undefined = -1 whatever -undefined-out
// says; the labels become floats, -1 the largest label plus one (or the -undefined-out value), and voxels outside the
// mask take the -mask-out value below like every other output
void handle_watershed(Run& r) {
  const Settings& s = r.s;
  const size_t n = r.tomo_in.nvox();
  vector<int32_t> labels(n), markers;
  if (!s.watershed_markers_filename.empty()) {
    Mrc mk;
    cerr << "Reading tomogram \"" << s.watershed_markers_filename << "\"\n";
    mk.read(s.watershed_markers_filename);
    if (mk.nx != r.size[0] || mk.ny != r.size[1] || mk.nz != r.size[2])
      throw VisfdErr("Error: \"" + s.watershed_markers_filename + "\" does not have the size of the input image.\n");
    markers.resize(n);
    for (size_t i = 0; i < n; i++) markers[i] = (int32_t)std::round(mk.data()[i]);
  }
  Table3D<int32_t> dest, mark;
  dest.alloc(r.size);
  if (!markers.empty()) {
    mark.alloc(r.size);
    std::memcpy(&mark.a[0][0][0], markers.data(), n * 4);
  }
  vector<std::array<float, 3> > extrema_crds;
  vector<float> extrema_scores;
  const size_t num_basins =
      Watershed(r.size, r.tomo_in.a, dest.a, r.mask3d(), static_cast<int32_t const* const* const*>(mark.a),
                s.watershed_threshold, !s.clusters_begin_at_maxima, s.neighbor_connectivity, s.watershed_show_boundaries,
                (int32_t)s.watershed_boundary_label, (int32_t)-1, &extrema_crds, &extrema_scores, &cerr);
  cerr << "Number of basins found: " << num_basins << "\n";
  const int32_t* lab = &dest.a[0][0][0];
  int32_t max_label = lab[0];
  for (size_t i = 0; i < n; i++) max_label = std::max(max_label, lab[i]);
  labels_to_image(s, lab, max_label, r.tomo_out.data(), n);
}

// the vote tensors (six channels per voxel, when anything below needs them) and the saliency in tomo_out: detected, or
// loaded from the files of an earlier -save-progress
void detect_or_load_tensors(Run& r, int order, vector<float>& tensor) {
  const Settings& s = r.s;
  const size_t n = r.tomo_in.nvox();
  const float* mptr = r.mask_flat();
  if (s.load_base.empty()) {
    float thr = 0;
    hip_detail::check(visfd_hip_membrane_detect_bg(
        hip_detail::context(), r.tomo_in.data(), mptr, r.size[0], r.size[1], r.size[2],
        s.width_a[0], r.ratio, order, s.hessian_thr_is_fraction ? s.hessian_thr : -1.0f, s.hessian_thr, s.tv_sigma,
        s.tv_exponent, s.tv_truncate, s.width_b[0] > 0.0f ? s.width_b[0] : 0.0f, s.normalize ? 1 : 0, r.tomo_out.data(),
        tensor.empty() ? nullptr : tensor.data(), nullptr, &thr));
    cerr << "  (saliency threshold = " << thr << ")\n";
  } else {
    // handlers.cpp:1840-1862: the vote tensors come from "<base>_tensor_<d>.rec" (written by -save-progress)
    for (int c = 0; c < 6; c++) {
      std::ostringstream name;
      name << s.load_base << "_tensor_" << c << ".rec";
      cerr << "loading \"" << name.str() << "\"\n";
      Mrc t;
      t.read(name.str());
      if (t.nx != r.size[0] || t.ny != r.size[1] || t.nz != r.size[2])
        throw VisfdErr("Error: \"" + name.str() + "\" does not have the size of the (binned) input image.\n");
      const float* p = t.data();
      for (size_t i = 0; i < n; i++)
        if (!mptr || mptr[i] != 0.0f) tensor[6 * i + c] = p[i];
    }
    hip_detail::check(visfd_hip_tensor_saliency_host(tensor.data(), mptr, (int64_t)n, order, r.tomo_out.data()));
    if (s.width_b[0] > 0.0f) {   // the peak-height factor of the post-vote loop, handlers.cpp:1577-1592,1883-1887
      Mrc bgv;
      bgv.alloc(r.size[0], r.size[1], r.size[2]);
      const float sb[3] = {s.width_b[0], s.width_b[0], s.width_b[0]};
      const int hb = (int)std::floor(s.width_b[0] * r.ratio);
      const int hwb[3] = {hb, hb, hb};
      hip_detail::check(visfd_hip_apply_gauss(hip_detail::context(), r.tomo_in.data(), bgv.data(), mptr, r.size[0], r.size[1], r.size[2], sb, hwb,
                                              s.normalize ? 1 : 0, nullptr));
      const float* img = r.tomo_in.data();
      const float* bg = bgv.data();
      float* o = r.tomo_out.data();
      for (size_t i = 0; i < n; i++)
        if (!mptr || mptr[i] != 0.0f) o[i] *= img[i] - bg[i];
    }
  }
}

void save_tensors(Run& r, const vector<float>& tensor) {
  const Settings& s = r.s;
  const size_t n = r.tomo_in.nvox();
  const float* mptr = r.mask_flat();
  Mrc t;
  t.alloc(r.size[0], r.size[1], r.size[2]);
  t.copy_header_from(r.tomo_in);
  // (the reference starts each tensor file from a copy of tomo_out: masked voxels keep its values)
  for (int c = 0; c < 6; c++) {
    float* o = t.data();
    const float* base = r.tomo_out.data();
    for (size_t i = 0; i < n; i++) o[i] = (!mptr || mptr[i] != 0.0f) ? tensor[6 * i + c] : base[i];
    std::ostringstream name;
    name << s.save_base << "_tensor_" << c << ".rec";
    cerr << "writing \"" << name.str() << "\"\n";
    t.write(name.str(), r.tomo_in);
  }
}

// -normals-file (handlers.cpp:2039-2309): the points of the selected cluster's surface and their normals, as a PLY file
// With a context (`ctx` non-null) the points come from the device in one call (visfd_hip_surface_points_ctx: the same points
// bit for bit, profiles/surface_points_time.txt); without a device the host entry counts, then fills.
void write_normals_file(Run& r, visfd_hip_ctx* ctx, const vector<float>& saliency, const vector<float>& direction) {
  const Settings& s = r.s;
  const float* mptr = r.mask_flat();
  const float* o = r.tomo_out.data();
  float maxd = s.max_distance_to_feature;                     // filter_mrc.cpp:301-307
  if (maxd < 0.0f) maxd /= -r.vw[0];
  else maxd /= (float)r.bin;
  int64_t np = 0;
  vector<float> crds, norms;
  if (ctx) {
    int64_t cap = 1 << 16;
    for (int attempt = 0; attempt < 2; attempt++) {   // too small a guess: the count comes back, once more with room for it
      crds.assign(3 * (size_t)cap + 3, 0.0f);
      norms.assign(3 * (size_t)cap + 3, 0.0f);
      const int rc = visfd_hip_surface_points_ctx(ctx, saliency.data(), o, direction.data(), mptr, r.size[0], r.size[1], r.size[2],
                                                  s.select_cluster, r.vw, s.surface_normal_curve_ds,
                                                  s.surface_find_ridge ? 1 : 0, maxd, crds.data(), norms.data(), cap, &np);
      if (rc == VISFD_HIP_ECAPACITY && attempt == 0) { cap = np; continue; }
      hip_detail::check(rc);
      break;
    }
  } else {
    hip_detail::check(visfd_hip_surface_points(saliency.data(), o, direction.data(), mptr, r.size[0], r.size[1], r.size[2],
                                               s.select_cluster, r.vw, s.surface_normal_curve_ds, s.surface_find_ridge ? 1 : 0,
                                               maxd, nullptr, nullptr, 0, &np));
    crds.assign(3 * (size_t)np + 3, 0.0f);
    norms.assign(3 * (size_t)np + 3, 0.0f);
    hip_detail::check(visfd_hip_surface_points(saliency.data(), o, direction.data(), mptr, r.size[0], r.size[1], r.size[2],
                                               s.select_cluster, r.vw, s.surface_normal_curve_ds, s.surface_find_ridge ? 1 : 0,
                                               maxd, crds.data(), norms.data(), np, &np));
  }
  std::ofstream ply(s.out_normals_file.c_str());              // file_io.hpp:501-527
  if (!ply) throw VisfdErr("Error: unable to open \"" + s.out_normals_file + "\" for writing.\n");
  ply << "ply\nformat ascii 1.0\ncomment  created by visfd\nelement vertex " << np
      << "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
         "property float nz\nend_header\n";
  for (int64_t k = 0; k < np; k++)
    ply << crds[3 * k] << " " << crds[3 * k + 1] << " " << crds[3 * k + 2] << " " << norms[3 * k] << " "
        << norms[3 * k + 1] << " " << norms[3 * k + 2] << "\n";
}

// visfd_hip_label_connected_ex behind the signature of visfd_hip_label_connected_device_seeds
int connect_on_host(visfd_hip_ctx*, const float* saliency, int64_t* labels, const float* mask, int64_t nx, int64_t ny,
                    int64_t nz, float ts, float* direction, float tvs, float tvn, int signs, const float* tensor, float tts,
                    float ttn, int posdef, int connectivity, int64_t label_undefined, int sort_by_size, int standardize,
                    int from_maxima, int64_t* n_clusters, float* cm, float* cs, float* csal, int64_t cap, const float* weights,
                    const float* ml_crds, const int64_t* ml_sizes, int64_t ml_n, const int* ml_dirs) {
  return visfd_hip_label_connected_ex(saliency, labels, mask, nx, ny, nz, ts, direction, tvs, tvn, signs, tensor, tts, ttn,
                                      posdef, connectivity, label_undefined, sort_by_size, standardize, from_maxima, n_clusters,
                                      cm, cs, csal, cap, weights, ml_crds, ml_sizes, ml_n, ml_dirs);
}

// -connect (handlers.cpp:1925-2035).  Saliency and directions are recomputed on the host in the reference's own
// arithmetic (the flood order and the angle thresholds act on them); the vote tensors are exact already.
void cluster(Run& r, int order, const vector<float>& tensor) {
  const Settings& s = r.s;
  const size_t n = r.tomo_in.nvox();
  const float* mptr = r.mask_flat();
  hip_detail::check(visfd_hip_tensor_saliency_host(tensor.data(), mptr, (int64_t)n, order, r.tomo_out.data()));
  vector<float> direction(3 * n, 0.0f);
  hip_detail::check(visfd_hip_principal_directions_host(tensor.data(), mptr, (int64_t)n, order, direction.data()));
  vector<int64_t> labels(n);
  int64_t n_clusters = 0;
  // -load-progress ... -connect needs no GPU for anything else: on a machine without a device the seeds are searched on
  // the host as well.  Any other failure to get a context (a bad VISFD_HIP_DEVICE, a driver or memory error) is reported
  // like everywhere else in this program.
  visfd_hip_ctx* ctx = nullptr;
  try {
    ctx = hip_detail::context();
  } catch (const VisfdErr& e) {
    if (std::string(e.what()).find("no HIP device available") == std::string::npos) throw;
  }
  // With a device: the graph entry, with must-links and doubtful outward sums settled on its device path (option
  // connect_settle); labels and the directions of labelled voxels are the flood's bits, and nothing below reads any other
  // direction.  The option is put back afterwards: the context is the program's one.
  int64_t settle_before = 0;
  if (ctx) {
    hip_detail::check(visfd_hip_get_option(ctx, "connect_settle", &settle_before));
    hip_detail::check(visfd_hip_set_option(ctx, "connect_settle", 1));
  }
  hip_detail::check((ctx ? visfd_hip_label_connected_graph : connect_on_host)(   // the same labels either way
      ctx, r.tomo_out.data(), labels.data(), mptr, r.size[0], r.size[1], r.size[2], s.connect_threshold_saliency,
      direction.data(), s.connect_threshold_vector_saliency, s.connect_threshold_vector_neighbor, 0, tensor.data(),
      s.connect_threshold_tensor_saliency, s.connect_threshold_tensor_neighbor, 1, 1, -1, 1, 1, 1, &n_clusters,
      nullptr, nullptr, nullptr, 0, nullptr, s.must_link_crds.empty() ? nullptr : s.must_link_crds.data(),
      s.must_link_group_sizes.empty() ? nullptr : s.must_link_group_sizes.data(),
      (int64_t)s.must_link_group_sizes.size(), s.must_link_directions.empty() ? nullptr : s.must_link_directions.data()));
  if (ctx) hip_detail::check(visfd_hip_set_option(ctx, "connect_settle", settle_before));
  cerr << "Number of clusters found: " << n_clusters << "\n";
  int64_t max_label = labels[0];
  for (size_t i = 0; i < n; i++)
    if (!mptr || mptr[i] != 0.0f) max_label = std::max(max_label, labels[i]);
  vector<float> saliency;
  if (!s.out_normals_file.empty()) saliency.assign(r.tomo_out.data(), r.tomo_out.data() + n);   // handlers.cpp:1929-1934
  labels_to_image(s, labels.data(), max_label, r.tomo_out.data(), n);
  if (!s.out_normals_file.empty()) write_normals_file(r, ctx, saliency, direction);
}

bool handle_membrane(Run& r) {
  const Settings& s = r.s;
  cerr << "filter_type = surface ridge detector\n";
  const int order = s.ridges_are_maxima ? VISFD_HIP_INCREASING_EIVALS : VISFD_HIP_DECREASING_EIVALS;  // handlers.cpp:1524-1535
  if (s.slab_world > 0) {
    membrane_slab(r, order);
    return false;
  }
  const size_t n = r.tomo_in.nvox();
  const bool want_tensor = s.tv_sigma > 0 && (!s.save_base.empty() || s.cluster_connected_voxels || !s.load_base.empty());
  vector<float> tensor(want_tensor ? 6 * n : 0);
  detect_or_load_tensors(r, order, tensor);
  if (!tensor.empty() && !s.save_base.empty()) save_tensors(r, tensor);
  if (s.cluster_connected_voxels) cluster(r, order, tensor);
  return true;
}

// -cl (handlers.cpp:1015-1032): AverageArr and StdDevArr add in float, weighted by the mask's values, in scan order
// (visfd_utils.hpp:685-790).  Such sums depend on their order by nature, so they are formed here, on the host, in that order.
void clipping_sigma_thresholds(Run& r, float* a, float* b) {
  const float* h = r.tomo_in.data();
  const float* w = r.mask_flat();
  const size_t n = r.tomo_in.nvox();
  float total = 0.0f, denom = 0.0f;
  for (size_t i = 0; i < n; i++) {
    float x = h[i];
    if (w) { x *= w[i]; denom += w[i]; }
    else denom += 1.0f;
    total += x;
  }
  const float ave = total / denom;
  total = denom = 0.0f;
  for (size_t i = 0; i < n; i++) {
    float x = h[i] - ave;
    x *= x;
    if (w) { x *= w[i]; denom += w[i]; }
    else denom += 1.0f;
    total += x;
  }
  const float stddev = std::sqrt(total / denom);
  *a = ave + r.s.in_threshold_01_a * stddev;
  *b = ave + r.s.in_threshold_01_b * stddev;
  cerr << "ave=" << ave << ", stddev=" << stddev << std::endl;
  cerr << "  Clipping intensities between [" << *a << ", " << *b << "]" << std::endl;
}

// The reference's tail (filter_mrc.cpp:746-786): -invert, one intensity map, the -mask-out value outside the mask,
// -rescale-min-max, each where asked for, in at most one statistics pass and two map passes on the device.
void intensity_tail(Run& r, bool mask_fill) {
  const Settings& s = r.s;
  visfd_hip_ctx* ctx = hip_detail::context();
  float* out = r.tomo_out.data();
  const float* mp = r.mask_flat();
  const size_t n = r.tomo_out.nvox();
  const int64_t nx = r.tomo_out.nx, ny = r.tomo_out.ny, nz = r.tomo_out.nz;
  visfd_hip_intensity p;
  std::memset(&p, 0, sizeof(p));
  if (s.invert_output) {   // MrcSimple::Invert: about the mean of the voxels inside the mask
    visfd_hip_stats st;
    hip_detail::check(visfd_hip_image_stats(ctx, out, mp, (int64_t)n, &st));
    p.invert = 1;
    if (st.n_nonfinite == 0 && st.order_free) p.ave = st.sum / (double)st.count;
    else {
      cerr << "-invert: summing on the host in scan order (no proof that the sum of this image is the same in every order)\n";
      double sum = 0.0;
      long cnt = 0;
      for (size_t i = 0; i < n; i++)
        if (!mp || mp[i] != 0.0f) { sum += out[i]; cnt++; }
      p.ave = sum / cnt;
    }
  }
  if (s.use_intensity_map) {   // HandleThresholds, handlers.cpp:1003-1081
    cerr << "Applying thresholds" << std::endl;
    p.out_a = s.out_thresh_a_value;
    p.out_b = s.out_thresh_b_value;
    if (s.use_rescale_multiply) {
      p.map = VISFD_HIP_MAP_RESCALE;
      p.t[0] = s.out_rescale_multiply; p.t[1] = s.out_rescale_offset;
    } else if (s.use_gauss_thresholds) {
      p.map = VISFD_HIP_MAP_GAUSS;
      p.t[0] = s.out_thresh_gauss_x0; p.t[1] = s.out_thresh_gauss_sigma;
    } else if (!s.use_dual_thresholds) {
      float a = s.in_threshold_01_a, b = s.in_threshold_01_b;
      if (s.out_thresh2_use_clipping_sigma) clipping_sigma_thresholds(r, &a, &b);
      p.t[0] = a; p.t[1] = b;
      if (a == b) p.map = VISFD_HIP_MAP_STEP;
      else {
        p.map = VISFD_HIP_MAP_THRESH2;
        if (s.out_thresh2_use_clipping) { p.out_a = a; p.out_b = b; }
      }
    } else {
      p.map = VISFD_HIP_MAP_THRESH4;
      p.t[0] = s.in_threshold_01_a; p.t[1] = s.in_threshold_01_b; p.t[2] = s.in_threshold_10_a; p.t[3] = s.in_threshold_10_b;
    }
    if (s.threshold_map() && (s.type != Settings::NONE || s.invert_output))
      cerr << "NOTE: " << s.threshold_flag << " maps the INPUT image, as in the reference: what the filter"
           << (s.invert_output ? " and -invert" : "") << " wrote to the output is overwritten.\n";
  }
  if (mask_fill) { p.mask_fill = 1; p.masked_value = s.masked_voxel_brightness; }
  const bool one_pass = p.invert || p.map != VISFD_HIP_MAP_NONE || p.mask_fill;
  if (!s.rescale_min_max_out) {
    if (one_pass) hip_detail::check(visfd_hip_intensity_map(ctx, r.tomo_in.data(), out, mp, nx, ny, nz, &p, nullptr));
    return;
  }
  // MrcSimple::Rescale01: the extremes of what the stages above leave inside the mask, then every voxel
  visfd_hip_stats st;
  p.stats_mask = 1;
  if (one_pass) hip_detail::check(visfd_hip_intensity_map(ctx, r.tomo_in.data(), out, mp, nx, ny, nz, &p, &st));
  else hip_detail::check(visfd_hip_image_stats(ctx, out, mp, (int64_t)n, &st));
  float dmin = st.min, dmax = st.max;
  if (st.n_nonfinite != 0) {   // FindMinMaxMean's comparisons in scan order (mrc_simple.cpp:396-424)
    double lo = 0.0, hi = -1.0;
    for (size_t i = 0; i < n; i++) {
      if (mp && mp[i] == 0.0f) continue;
      if (lo > hi) lo = hi = out[i];
      else { if (out[i] > hi) hi = out[i]; if (out[i] < lo) lo = out[i]; }
    }
    dmin = (float)lo; dmax = (float)hi;
  }
  visfd_hip_intensity q;
  std::memset(&q, 0, sizeof(q));
  q.rescale01 = 1;
  q.dmin = dmin; q.dmax = dmax;
  q.rescale_a = s.out_rescale_min; q.rescale_b = s.out_rescale_max;
  hip_detail::check(visfd_hip_intensity_map(ctx, nullptr, out, nullptr, nx, ny, nz, &q, nullptr));
}

// What ends every run but a -slab one: back to the input's size, the reference's tail (-invert, an intensity map, the
// -mask-out value outside the mask, -rescale-min-max), the output file
void finish(Run& r) {
  const Settings& s = r.s;
  if (s.type == Settings::SURFACE_RIDGE && r.bin > 1 && !s.bin_explicit) {   // handlers.cpp:2315-2355
    r.tomo_out.loaded = true;
    r.tomo_out.copy_header_from(r.tomo_in);   // (the cell is set by unbin_image)
    unbin_image(r.tomo_out, r.size_orig, r.cella_orig);
    unbin_image(r.tomo_in, r.size_orig, r.cella_orig);   // only its header/size is used below
    if (r.mask.loaded) unbin_image(r.mask, r.size_orig, r.cella_orig);
  }
  // filter_mrc.cpp:765-776: after everything else, voxels outside the mask take the "masked" brightness
  if (s.has_tail()) intensity_tail(r, r.mask.loaded && s.type != Settings::BLOB_NONMAX);
  else if (r.mask.loaded && s.type != Settings::BLOB_NONMAX) {
    float* o = r.tomo_out.data();
    const float* mp = r.mask.data();
    for (size_t i = 0; i < r.tomo_out.nvox(); i++)
      if (mp[i] == 0.0f) o[i] = s.masked_voxel_brightness;
  }
  if (!s.out.empty()) {
    cerr << "writing tomogram (in 32-bit float mode)\n";
    r.tomo_out.write(s.out, r.tomo_in);
  }
}

}  // namespace

int main(int argc, char** argv) {
  try {
    cerr << "filter_mrc (visfd-mi355x, hot path on libvisfd_hip ABI " << visfd_hip_abi_version() << ")\n";
    Settings s = parse(argc, argv);
    Run r(s);
    load(r);
    prepare(r, s);
    bool whole_image = true;   // false after a -slab run: the handler has written this rank's planes
    switch (s.type) {
      case Settings::NONE: break;
      case Settings::GAUSS: whole_image = handle_gauss(r); break;
      case Settings::LOCAL_FLUCTUATIONS: handle_fluctuations(r); break;
      case Settings::GGAUSS: handle_ggauss(r); break;
      case Settings::DOGG: handle_dogg(r); break;
      case Settings::DOG: handle_dog(r); break;
      case Settings::LOG: handle_log(r); break;
      case Settings::BLOB: handle_blob(r); break;
      case Settings::MORPHOLOGY: handle_morphology(r); break;
      case Settings::FIND_EXTREMA: handle_extrema(r); break;
      case Settings::WATERSHED: handle_watershed(r); break;
      case Settings::BLOB_NONMAX: handle_blob_nonmax(r); break;
      case Settings::BLOB_NONMAX_SUPERVISED_MULTI: handle_supervised_multi(r); break;
      case Settings::DRAW_SPHERES: handle_draw_spheres(r); break;
      case Settings::DISTANCE_TO_POINTS: handle_distance_points(r); break;
      case Settings::DISTANCE_TO_VOXELS: handle_distance_to_voxels(r); break;
      case Settings::SURFACE_RIDGE: whole_image = handle_membrane(r); break;
    }
    if (whole_image) finish(r);
  } catch (std::exception& e) {
    cerr << "\n" << e.what() << std::endl;
    return 1;
  }
  return 0;
}
