// fra_api.hip -- the C ABI (include/flac_raster_amd.h) outside the plan: errors, contexts, the stream header,
// fra_normalize, the synthetic rasters, device / page-locked memory and the one-call fra_encode.  The plan lives in
// fra_plan.hip, fra_plan_execute in fra_exec.hip, the host pipeline in fra_hostpath.hip.  No kernels here.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "fra_plan.h"

namespace fra {
hipError_t launch_synth(int kind, uint64_t seed, int bands, int H, int W, void* out, hipStream_t s);
hipError_t launch_normalize_flat(int src, const void* data, uint64_t n, int bps, NormDev* nd, int has_min, double omin,
                                 int has_max, double omax, void* out, hipStream_t s);
}  // namespace fra

using namespace fra;

static thread_local std::string g_err;

static const char kVendor[] = "flac-raster-amd 0.1.0 gfx950 HIP";  // 32 bytes, as libFLAC's vendor string

extern "C" {

int fra_internal_set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// device and stream of a context, for the translation units that do not see fra_ctx (fra_decode_dev.hip)
void fra_internal_ctx_stream(fra_ctx* ctx, int* device, hipStream_t* stream) {
  *device = ctx->device;
  *stream = ctx->stream;
}

const char* fra_last_error(void) { return g_err.c_str(); }
int fra_abi_version(void) { return FRA_ABI_VERSION; }
void fra_free(void* p) { free(p); }

int fra_device_count(int* count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *count = n;
  return FRA_OK;
}

int fra_ctx_create(int device, fra_ctx** out) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return set_err(FRA_E_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return set_err(FRA_E_INVALID, "device %d out of range (%d devices)", device, n);
  HIPCHK(hipSetDevice(device));
  fra_ctx* c = new (std::nothrow) fra_ctx();
  if (!c) return set_err(FRA_E_NOMEM, "out of host memory");
  c->device = device;
  // the highest stream priority: background kernels of pipelined plans (low-priority streams) fill the
  // CU resources k_analyze leaves free rather than competing for them
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
  hipError_t e = c->res.stream(&c->stream, hi);
  if (e != hipSuccess) { delete c; return set_err(FRA_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
  *out = c;
  return FRA_OK;
}

void fra_ctx_destroy(fra_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

int fra_host_alloc(uint64_t bytes, void** ptr) {
  if (!ptr) return set_err(FRA_E_INVALID, "null argument");
  *ptr = nullptr;
  HIPCHK(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocPortable));
  return FRA_OK;
}
int fra_host_free(void* ptr) {
  if (ptr) HIPCHK(hipHostFree(ptr));
  return FRA_OK;
}
int fra_host_register(void* ptr, uint64_t bytes) {
  if (!ptr || !bytes) return set_err(FRA_E_INVALID, "null argument");
  HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterPortable));
  return FRA_OK;
}
int fra_host_unregister(void* ptr) {
  if (ptr) HIPCHK(hipHostUnregister(ptr));
  return FRA_OK;
}

int fra_encode(int device, const fra_job* job, uint8_t** out, uint64_t* out_len, fra_stream_info* infos) {
  fra_ctx* ctx = nullptr;
  int rc = fra_ctx_create(device, &ctx);
  if (rc) return rc;
  fra_plan* p = nullptr;
  rc = fra_plan_create(ctx, job, &p);
  if (!rc) rc = fra_plan_execute(p);
  if (!rc) rc = fra_plan_sync(p);
  uint64_t total = 0;
  if (!rc) rc = fra_plan_result(p, infos, &total);
  if (!rc) {
    *out = (uint8_t*)malloc(total ? total : 1);
    if (!*out) rc = set_err(FRA_E_NOMEM, "malloc %llu", (unsigned long long)total);
    else rc = fra_plan_download(p, *out, total);
    if (rc) { free(*out); *out = nullptr; }
    *out_len = total;
  }
  KeepError keep;
  fra_plan_destroy(p);
  fra_ctx_destroy(ctx);
  return rc;
}

int fra_stream_header(uint8_t* o, int32_t channels, int32_t bps, int32_t sample_rate, int32_t blocksize) {
  if (!o || channels < 1 || channels > 8 || bps < 4 || bps > 32 || blocksize < 16 || blocksize > 65535 ||
      sample_rate <= 0 || sample_rate >= (1 << 20))
    return set_err(FRA_E_INVALID, "bad stream header parameters");
  memcpy(o, "fLaC", 4);
  o[4] = 0x00;  // STREAMINFO, not last
  o[5] = 0; o[6] = 0; o[7] = 34;
  uint8_t* si = o + 8;
  memset(si, 0, 34);
  si[0] = (uint8_t)(blocksize >> 8); si[1] = (uint8_t)blocksize;
  si[2] = (uint8_t)(blocksize >> 8); si[3] = (uint8_t)blocksize;
  // bytes 4..9 min/max frame size = 0
  // 20-bit sample rate | 3-bit channels-1 | 5-bit bps-1 | 36-bit total samples (0)
  si[10] = (uint8_t)(sample_rate >> 12);
  si[11] = (uint8_t)(sample_rate >> 4);
  si[12] = (uint8_t)(((sample_rate & 0xF) << 4) | ((channels - 1) << 1) | ((bps - 1) >> 4));
  si[13] = (uint8_t)(((bps - 1) & 0xF) << 4);
  // MD5 zero
  uint8_t* vc = o + 42;
  const uint32_t vlen = (uint32_t)(sizeof(kVendor) - 1);
  const uint32_t blen = 4 + vlen + 4;
  vc[0] = 0x84;  // last | VORBIS_COMMENT
  vc[1] = (uint8_t)(blen >> 16); vc[2] = (uint8_t)(blen >> 8); vc[3] = (uint8_t)blen;
  vc[4] = (uint8_t)vlen; vc[5] = (uint8_t)(vlen >> 8); vc[6] = (uint8_t)(vlen >> 16); vc[7] = (uint8_t)(vlen >> 24);
  memcpy(vc + 8, kVendor, vlen);
  memset(vc + 8 + vlen, 0, 4);
  return FRA_OK;  // 42 + 4 + 40 = 86 bytes
}

int fra_normalize(fra_ctx* ctx, const void* data, int32_t on_device, int32_t dtype, uint64_t n, int32_t bps,
                  const double* data_min, const double* data_max, void* out_host, double* mn_out, double* mx_out) {
  if (!ctx || (!data && n) || (!out_host && n)) return set_err(FRA_E_INVALID, "null argument");
  if (dtype < FRA_U8 || dtype > FRA_F64) return set_err(FRA_E_INVALID, "bad dtype %d", dtype);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  const size_t in_bytes = (size_t)n * elem_size(dtype);
  const size_t out_bytes = (size_t)n * (bps == 16 ? 2 : 4);
  HipArena res;  // this call's device buffers
  void* d_in = nullptr;
  void* d_out = nullptr;
  NormDev* d_nd = nullptr;
  if (!on_device && n) {
    HIPCHK(res.alloc(&d_in, in_bytes));
    HIPCHK(hipMemcpyAsync(d_in, data, in_bytes, hipMemcpyHostToDevice, s));
  }
  HIPCHK(res.alloc(&d_out, std::max<size_t>(4, out_bytes)));
  HIPCHK(res.alloc(&d_nd, sizeof(NormDev)));
  HIPCHK(launch_normalize_flat(dtype, on_device ? data : d_in, n, bps, d_nd, data_min != nullptr,
                               data_min ? *data_min : 0.0, data_max != nullptr, data_max ? *data_max : 0.0, d_out, s));
  NormDev nd{};
  if (out_bytes) HIPCHK(hipMemcpyAsync(out_host, d_out, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&nd, d_nd, sizeof(NormDev), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (mn_out) *mn_out = nd.mn;
  if (mx_out) *mx_out = nd.mx;
  return FRA_OK;
}

int fra_synth_raster(fra_ctx* ctx, int32_t kind, uint64_t seed, int32_t bands, int32_t height, int32_t width,
                     void* dev_out) {
  if (!ctx || !dev_out || bands < 1 || height < 1 || width < 1 || (kind != 3 && kind != 4 && kind != 5))
    return set_err(FRA_E_INVALID, "bad synth arguments");
  (void)hipSetDevice(ctx->device);
  HIPCHK(launch_synth(kind, seed, bands, height, width, dev_out, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FRA_OK;
}

int fra_device_alloc(fra_ctx* ctx, uint64_t bytes, void** p) {
  (void)hipSetDevice(ctx->device);
  HIPCHK(hipMalloc(p, bytes ? bytes : 1));
  return FRA_OK;
}
int fra_device_free(fra_ctx* ctx, void* p) {
  (void)hipSetDevice(ctx->device);
  HIPCHK(hipFree(p));
  return FRA_OK;
}
int fra_memcpy_d2h(fra_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  (void)hipSetDevice(ctx->device);
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return FRA_OK;
}
int fra_memcpy_h2d(fra_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  (void)hipSetDevice(ctx->device);
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return FRA_OK;
}

}  // extern "C"
