// context.hip -- the context behind the C ABI: the error string, the workspace slots, the option table, and the
// entry points that create, query, trim and destroy a context.
#include <cctype>
#include <cstdlib>

#include "common.hpp"

namespace vh {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int ws_get(visfd_hip_ctx* ctx, Slot s, size_t bytes, void** out) {
  if (bytes == 0) bytes = 16;
  if (ctx->slot_bytes[s] < bytes) {
    ctx->slot_key[s].clear();   // the contents go with the buffer
    // a queued blob scan that nobody has collected yet writes its survivors and counts here: fetch them first
    if (ctx->slot_ptr[s] && (s == WS_CAND || s == WS_SCANCNT)) VH_TRY(blob_jobs_drain(ctx));
    if (ctx->slot_ptr[s]) {
      // buffers may still be in use by queued kernels
      VH_HIP(hipStreamSynchronize(ctx->stream));
      VH_HIP(hipFree(ctx->slot_ptr[s]));
      ctx->slot_ptr[s] = nullptr;
      ctx->slot_bytes[s] = 0;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess)
      return fail(VISFD_HIP_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed: " +
                                        hipGetErrorString(e));
    ctx->slot_ptr[s] = p;
    ctx->slot_bytes[s] = bytes;
  }
  *out = ctx->slot_ptr[s];
  return VISFD_HIP_OK;
}

bool ws_holds(const visfd_hip_ctx* ctx, Slot s, const void* key, size_t key_bytes) {
  const std::vector<unsigned char>& k = ctx->slot_key[s];
  return key_bytes > 0 && k.size() == key_bytes && std::memcmp(k.data(), key, key_bytes) == 0;
}

int ws_put(visfd_hip_ctx* ctx, Slot s, const void* key, size_t key_bytes, const void* host, size_t bytes) {
  ctx->slot_key[s].clear();                    // until the new contents have arrived
  VH_HIP(hipStreamSynchronize(ctx->stream));   // queued kernels may still read what the slot holds now
  void* d = nullptr;
  VH_TRY(ws_get(ctx, s, bytes, &d));
  VH_HIP(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));   // the copy reads host memory of this call
  const unsigned char* k = static_cast<const unsigned char*>(key);
  ctx->slot_key[s].assign(k, k + key_bytes);
  return VISFD_HIP_OK;
}

namespace {

// ---- options: name -> field; VISFD_HIP_<NAME> in the environment gives the value a new context starts with ----------
struct OptionDesc {
  const char* name;
  int visfd_hip_options::*i = nullptr;
  int64_t visfd_hip_options::*l = nullptr;
  OptionDesc(const char* n, int visfd_hip_options::*f) : name(n), i(f) {}
  OptionDesc(const char* n, int64_t visfd_hip_options::*f) : name(n), l(f) {}
};
#define VH_OPT(field) {#field, &visfd_hip_options::field}
const OptionDesc kOptions[] = {   // every field of visfd_hip_options (common.hpp documents them), in its order
    VH_OPT(gauss_3pass), VH_OPT(gauss_cfg), VH_OPT(gauss_wg_per_cu), VH_OPT(log_pair), VH_OPT(log_pair_chunk),
    VH_OPT(membrane_queue),
    VH_OPT(tv_dense), VH_OPT(tv_fma), VH_OPT(gauss_fma), VH_OPT(eig_f32), VH_OPT(tv_zrun), VH_OPT(tv_no_replay),
    VH_OPT(tv_exact_tiled), VH_OPT(tv_no_fold), VH_OPT(tv_poison), VH_OPT(tv_reserve_wg), VH_OPT(tv_max_wg),
    VH_OPT(blob_test_cap), VH_OPT(morph_general), VH_OPT(morph_levels), VH_OPT(filter3d_general), VH_OPT(median_general),
    VH_OPT(distance_general), VH_OPT(discard_overlap_host), VH_OPT(discard_overlap_time),
    VH_OPT(discard_overlap_max_rounds), VH_OPT(find_spheres_host), VH_OPT(watershed_host), VH_OPT(stats_blocks),
    VH_OPT(connect_time), VH_OPT(connect_settle), VH_OPT(draw_time), VH_OPT(voxelize_bisect), VH_OPT(voxelize_time),
    VH_OPT(surface_steps_cap), VH_OPT(surface_points_time), VH_OPT(close_surface_rtol_exp),
    VH_OPT(close_surface_max_cycles), VH_OPT(close_surface_time), VH_OPT(isosurface_time), VH_OPT(debug),
};
#undef VH_OPT
bool set_option(visfd_hip_options* o, const char* name, int64_t value) {
  for (const OptionDesc& d : kOptions) {
    if (std::strcmp(d.name, name) != 0) continue;
    if (d.i) o->*(d.i) = (int)value; else o->*(d.l) = value;
    return true;
  }
  return false;
}
bool get_option(const visfd_hip_options* o, const char* name, int64_t* value) {
  for (const OptionDesc& d : kOptions) {
    if (std::strcmp(d.name, name) != 0) continue;
    *value = d.i ? (int64_t)(o->*(d.i)) : o->*(d.l);
    return true;
  }
  return false;
}
void options_from_environment(visfd_hip_options* o) {
  for (const OptionDesc& d : kOptions) {
    std::string env = "VISFD_HIP_";
    for (const char* c = d.name; *c; c++) env += (char)std::toupper((unsigned char)*c);
    if (const char* e = std::getenv(env.c_str())) set_option(o, d.name, (int64_t)std::atoll(e));
  }
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

// What each version added.  10: visfd_hip_blob_halo_depth (the blob halo in the kernels' float arithmetic); 9: BlobDog in
// two halves (visfd_hip_blob_dog_begin_dev / _end / _abort); 8: the peak-height factor (`-membrane-background`:
// visfd_hip_peak_background_dev, _ridge_scores_bg_dev, _tensor_saliency_bg_dev, _membrane_detect_bg[_dev],
// _membrane_detect_slab_bg[_dev]) and the program's slab Gaussian / blob entry points; 7: visfd_hip_membrane_detect_slab
// (host-memory face of the slab stage); 6: visfd_hip_get_option, tolerance modes (tv_fma, gauss_fma), slab entry points;
// 5: visfd_hip_set_option, CompactMultiChannelImage3D/TVDenseStick normalisation in the shim; 4: LocalFluctuations, two-step
// ridge (scores / directions); 3: host DiagonalizeFlatSym3 / ConvertFlatSym2Evects3; 2: blob post-processing, binning,
// LabelConnected and its host helpers.
int visfd_hip_abi_version(void) { return 10; }
const char* visfd_hip_last_error(void) { return g_last_error.c_str(); }

int visfd_hip_create(int device, void* stream, visfd_hip_ctx** out) {
  VH_REQUIRE(out, "null output pointer");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(VISFD_HIP_EDEVICE, "no HIP device available (libvisfd_hip has no CPU fallback)");
  VH_REQUIRE(device >= 0 && device < count, "bad device ordinal");
  VH_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  VH_HIP(hipGetDeviceProperties(&prop, device));
  visfd_hip_ctx* ctx = new visfd_hip_ctx();
  ctx->device = device;
  ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  options_from_environment(&ctx->opt);
  if (stream) {
    ctx->stream = (hipStream_t)stream;
    ctx->own_stream = false;
  } else {
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete ctx;
      return fail(VISFD_HIP_EDEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    ctx->own_stream = true;
  }
  *out = ctx;
  return VISFD_HIP_OK;
}

int visfd_hip_set_option(visfd_hip_ctx* ctx, const char* name, int64_t value) {
  VH_REQUIRE(ctx && name, "null argument");
  if (!set_option(&ctx->opt, name, value)) return fail(VISFD_HIP_EINVAL, std::string("unknown option: ") + name);
  return VISFD_HIP_OK;
}

int visfd_hip_get_option(visfd_hip_ctx* ctx, const char* name, int64_t* value) {
  VH_REQUIRE(ctx && name && value, "null argument");
  if (!get_option(&ctx->opt, name, value)) return fail(VISFD_HIP_EINVAL, std::string("unknown option: ") + name);
  return VISFD_HIP_OK;
}

int visfd_hip_trim(visfd_hip_ctx* ctx) {
  VH_REQUIRE(ctx, "null context");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(blob_jobs_drain(ctx));   // live blob jobs keep their lists on the host from here on
  VH_HIP(hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < WS_NSLOTS; s++) {
    ctx->slot_key[s].clear();
    if (ctx->slot_ptr[s]) VH_HIP(hipFree(ctx->slot_ptr[s]));
    ctx->slot_ptr[s] = nullptr;
    ctx->slot_bytes[s] = 0;
  }
  return VISFD_HIP_OK;
}

int visfd_hip_debug_poison_workspace(visfd_hip_ctx* ctx) {
  VH_REQUIRE(ctx, "null context");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(blob_jobs_drain(ctx));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < WS_NSLOTS; s++) {
    ctx->slot_key[s].clear();   // overwritten below
    if (ctx->slot_ptr[s]) VH_HIP(hipMemsetAsync(ctx->slot_ptr[s], 0xFF, ctx->slot_bytes[s], ctx->stream));
  }
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}

int visfd_hip_blob_jobs_pending(visfd_hip_ctx* ctx) { return ctx ? (int)ctx->blob_jobs.size() : 0; }

int visfd_hip_destroy(visfd_hip_ctx* ctx) {
  if (!ctx) return VISFD_HIP_OK;
  (void)hipSetDevice(ctx->device);
  blob_jobs_abort(ctx);
  int rc = visfd_hip_trim(ctx);
  if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
  if (ctx->stage_event) (void)hipEventDestroy(ctx->stage_event);
  if (ctx->stage_pinned) (void)hipHostFree(ctx->stage_pinned);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return rc;
}

void* visfd_hip_get_stream(visfd_hip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int visfd_hip_synchronize(visfd_hip_ctx* ctx) {
  VH_REQUIRE(ctx, "null context");
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}

int64_t visfd_hip_workspace_bytes(visfd_hip_ctx* ctx) {
  if (!ctx) return 0;
  int64_t t = 0;
  for (int s = 0; s < WS_NSLOTS; s++) t += (int64_t)ctx->slot_bytes[s];
  return t;
}

}  // extern "C"
