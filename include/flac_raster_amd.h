/*
 * flac_raster_amd.h -- C ABI of the MI355X (gfx950) FLAC raster encoder.
 *
 * This library replaces the encode half of the reference's pyflac/libFLAC boundary:
 *
 *   reference call site                                   what replaces it here
 *   ---------------------------------------------------   -------------------------------------
 *   pyflac.StreamEncoder(write_callback, sample_rate,     fra_encode() / fra_plan_*() with
 *     compression_level, blocksize=4096)                  fra_job.norm = 0 (samples are already
 *   encoder.process(audio); encoder.finish()              int16/int32 audio, pyflac semantics F3:
 *     src/flac_raster/converter.py:139-154                bps = itemsize*8)
 *     src/flac_raster/spatial_encoder.py:291-304
 *     (pyflac 3.0.0 _Encoder.process/finish,
 *      docs/sonos-pyflac.txt:1968-2014; libFLAC C ABI
 *      FLAC__stream_encoder_new, set_..., init_stream,
 *      process_interleaved/finish, :3205-3262)
 *
 *   normalize_to_audio(interleave(raster)) + the above,   fra_job.norm = 16 or 24: raw raster in,
 *     once per encode unit (whole raster / tile)          per-window nanmin/nanmax + the float64
 *     normalization.py:126-202, converter.py:93-154,      normalisation fused on the GPU
 *     spatial_encoder.py:196-245, cli.py:553-622
 *
 * Output of an encode = the FLAC *frames* of every window's stream, concatenated in window order,
 * plus per-stream info.  The 86-byte stream header (fLaC + STREAMINFO + VORBIS_COMMENT, F4 of
 * SURVEY.md) is produced by fra_stream_header(); the Python host layer assembles headers, tags
 * (mutagen-equivalent) and containers.
 *
 * Conventions: every function returns 0 on success or a negative fra_status; the message of the
 * last failure on the calling thread is fra_last_error().  No C++ exception crosses this ABI.
 * Library-allocated buffers are released with fra_free().  A context is bound to one HIP device
 * and owns one HIP stream; plans are not thread-safe, distinct plans may run on distinct threads.
 */
#ifndef FLAC_RASTER_AMD_H
#define FLAC_RASTER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRA_ABI_VERSION 3

#if defined(__GNUC__) || defined(__clang__)
#define FRA_API __attribute__((visibility("default")))
#else
#define FRA_API
#endif

typedef enum {
  FRA_OK = 0,
  FRA_E_INVALID = -1,   /* bad argument */
  FRA_E_HIP = -2,       /* HIP runtime error (message in fra_last_error) */
  FRA_E_NODEVICE = -3,  /* no usable gfx950 device */
  FRA_E_NOMEM = -4,
  FRA_E_STATE = -5,     /* call out of order (e.g. result before execute) */
  FRA_E_SPACE = -6      /* caller's output buffer too small (the required size is reported) */
} fra_status;

/* dtype codes of the source samples (numpy names) */
typedef enum {
  FRA_U8 = 0, FRA_I8 = 1, FRA_U16 = 2, FRA_I16 = 3, FRA_U32 = 4, FRA_I32 = 5, FRA_F32 = 6, FRA_F64 = 7
} fra_dtype;

/* one encode unit: a rasterio Window (cli.py:553-559 / spatial_encoder.py:110-121) */
typedef struct {
  int32_t row_off, col_off, height, width;
} fra_window;

typedef struct {
  const void *raster;       /* element (band 0, row 0, col 0) */
  int32_t raster_on_device; /* 1: device pointer on the context's GPU; 0: host memory (copied) */
  int32_t dtype;            /* fra_dtype */
  int32_t channels;         /* bands -> FLAC channels (1..8) */
  int64_t band_stride;      /* elements between bands */
  int64_t row_stride;       /* elements between rows */
  int64_t col_stride;       /* elements between pixels of a row (1 planar, C interleaved) */
  const fra_window *windows;
  int32_t nwindows;
  int32_t level;            /* FLAC compression level 0..8 (cli.py:60-62, default 5) */
  int32_t blocksize;        /* samples per frame, 16..4096 (reference passes 4096) */
  int32_t norm;             /* 0: samples already audio ints (pyflac path); 16 / 24: normalize_to_audio */
  int32_t sample_rate;      /* 0: calculate_audio_params rule from window H*W (normalization.py:108-120) */
  int32_t first_frame;      /* FLAC frame number of every stream's first frame (0; the pyflac shim
                               continues a stream across process() calls, sonos-pyflac.txt:1968-2001) */
} fra_job;

typedef struct {
  uint64_t offset;          /* byte offset of this stream's frames in the concatenated output */
  uint64_t frame_bytes;     /* bytes of frames (header excluded) */
  double data_min, data_max;/* normalize_to_audio params (NaN if all-NaN); 0/0 when norm == 0 */
  int32_t sample_rate, bps, channels, nframes;
} fra_stream_info;

typedef struct fra_ctx fra_ctx;
typedef struct fra_plan fra_plan;

FRA_API const char *fra_last_error(void);
FRA_API int fra_abi_version(void);
FRA_API int fra_device_count(int *count);
FRA_API void fra_free(void *p);

FRA_API int fra_ctx_create(int device, fra_ctx **out);
FRA_API void fra_ctx_destroy(fra_ctx *ctx);

/* Plan = all device workspace for one job shape; execute enqueues only (no allocation/sync). */
FRA_API int fra_plan_create(fra_ctx *ctx, const fra_job *job, fra_plan **out);
/* The same plan over FRAME RANGES of the windows (r05, multi-GPU work items of equal size):
 * frame_ranges[2 w] = first frame, frame_ranges[2 w + 1] = frame count (-1: to the stream's end) of window
 * w.  The normalisation (data_min/max, sample rate) still spans the whole window and the frames keep their
 * frame numbers, so the concatenated frames of all ranges of one window, in order, are exactly the stream
 * fra_plan_create would encode (the reference encodes a window as one stream, cli.py:553-597).
 * fra_stream_info.nframes / frame_bytes describe the range.  A count past the stream's end is clipped to it; a
 * first frame < 0 or past the stream's frame count, or a count < -1, is FRA_E_INVALID. */
FRA_API int fra_plan_create_ranged(fra_ctx *ctx, const fra_job *job, const int32_t *frame_ranges, fra_plan **out);
FRA_API int fra_plan_set_raster(fra_plan *plan, const void *raster, int32_t raster_on_device);
FRA_API int fra_plan_execute(fra_plan *plan);
FRA_API int fra_plan_sync(fra_plan *plan);
/* after sync: per-window info (array of plan's nwindows) and total output bytes */
FRA_API int fra_plan_result(fra_plan *plan, fra_stream_info *infos, uint64_t *total_bytes);
/* after sync: copy the concatenated frames (total_bytes) to host memory */
FRA_API int fra_plan_download(fra_plan *plan, uint8_t *host_out, uint64_t capacity);
/* device pointer of the concatenated frames (valid until the next execute / destroy) */
FRA_API int fra_plan_device_output(fra_plan *plan, const uint8_t **dev_ptr, uint64_t *capacity);
/* after sync: byte offset of every frame of the concatenated output, frames of all windows in
 * window order; offsets[nframes] = total bytes.  n must be sum(infos[].nframes) + 1.  This is what
 * the pyflac-compatible shim needs to replay libFLAC's one-write-callback-per-frame sequence
 * (docs/sonos-pyflac.txt:2311-2332). */
FRA_API int fra_plan_frame_offsets(fra_plan *plan, uint64_t *offsets, uint64_t n);
/* per-kernel timing with HIP events on the plan's stream: 0 minmax, 1 analyze, 2 frame-bytes+scan, 3 pack */
FRA_API int fra_plan_enable_timing(fra_plan *plan, int32_t on);
FRA_API int fra_plan_timing(fra_plan *plan, float *ms_sum4, int32_t *executes);
FRA_API void fra_plan_destroy(fra_plan *plan);

/* Host-resident raster -> host-resident frames in one pipelined pass (the PCIe-inclusive path that
 * replaces rasterio read -> pyflac encode -> file write per tile, cli.py:553-602 / converter.py:73-154).
 * The windows are grouped into row bands; the raster rows of band b are copied H2D on a copy stream
 * while the kernels of band b-1 run on the plan's stream, and band b's frames are copied D2H on a
 * second copy stream as soon as they are assembled (PCIe is full duplex).  host_raster has the job's
 * dtype and strides; host_raster and host_out should be page-locked (fra_host_alloc/fra_host_register)
 * for full link rate.  Frames land at the offsets fra_plan_result reports; *total_bytes = their sum.
 * If capacity < total, FRA_E_SPACE is returned (frames beyond capacity are not copied; the complete
 * output stays on the device for fra_plan_download).  Synchronous: returns when the frames are in
 * host_out.  A plan's capacity bound: fra_plan_capacity.
 * Layout contract of the three host entries (fra_plan_encode_host, _progress, fra_plan_encode_ring): rows are
 * copied as whole runs of row_stride elements, so the rows of a raster taller than one row must not overlap --
 * row_stride >= the elements one row spans, (C - 1) * col_stride + 1 with C the largest column end (col_off +
 * width) of the plan's windows, plus (channels - 1) * band_stride for an interleaved raster (band_stride <
 * row_stride).  A job with row_stride == 0 or any smaller stride than that (numpy broadcast or sliding views) is
 * refused with FRA_E_INVALID before any GPU work; fra_plan_create accepts it, and a device-resident raster
 * (fra_plan_execute) encodes it.  Padded rows, column offsets, pixel- and line-interleaved rasters are fine. */
FRA_API int fra_plan_encode_host(fra_plan *plan, const void *host_raster, uint8_t *host_out, uint64_t capacity,
                                 uint64_t *total_bytes);
/* The same pipelined pass over a raster that is still being produced (file-to-container path: a decoder
 * thread fills host_raster top to bottom, cli.py:553-559 reads each tile's window before its encode):
 * before the H2D copy of a row band is enqueued, the call waits until *rows_ready >= the band's last row
 * + 1 (the producer publishes rows with a release store; -1 = the producer failed: FRA_E_STATE).  Rows
 * are image rows of the job's raster (row_stride units).  Contract: the producer MUST eventually publish
 * either every row or -1 (also when it fails or is cancelled); the call waits without a time limit. */
FRA_API int fra_plan_encode_host_progress(fra_plan *plan, const void *host_raster, uint8_t *host_out, uint64_t capacity,
                                          uint64_t *total_bytes, const volatile int64_t *rows_ready);
/* The same pass with BOUNDED host memory for the raster (r05): the producer decodes into a ring of
 * ring_rows rows per channel instead of the whole raster -- image row r of channel c lives at ring row
 * r % ring_rows, the ring laid out (channels, ring_rows, row_stride) in the job's dtype (row_stride and
 * col_stride as in the job; channel c at c * ring_rows * row_stride elements; pixel-interleaved jobs use
 * one run).  *rows_ready as above; the call publishes in *rows_done (release store) the rows whose H2D copy
 * has completed: the producer may write image row r once r < *rows_done + ring_rows.  ring_rows must hold
 * the tallest host band (fra_plan_host_band_rows) plus the producer's own step, else FRA_E_INVALID.
 * Replaces the reference's per-tile window read (cli.py:553-559), which also never holds the raster. */
FRA_API int fra_plan_encode_ring(fra_plan *plan, const void *ring, int64_t ring_rows, uint8_t *host_out,
                                 uint64_t capacity, uint64_t *total_bytes, const volatile int64_t *rows_ready,
                                 volatile int64_t *rows_done);
/* rows of the tallest host band of a plan (the ring of fra_plan_encode_ring must hold it) */
FRA_API int fra_plan_host_band_rows(fra_plan *plan, int64_t *max_rows);
/* frame number of every stream's first frame for the next execute (the job's first_frame until set) */
FRA_API int fra_plan_set_first_frame(fra_plan *plan, int32_t first_frame);
/* upper bound of a plan's output bytes (every subframe VERBATIM + headers) and its number of host bands */
FRA_API int fra_plan_capacity(fra_plan *plan, uint64_t *capacity, int32_t *host_bands);
/* how the plan encodes (FRA_PLAN_*): PIPELINED = executes overlap (two or three sets of subframe slots, the
 * next execute's normalisation stage and this one's assembly run beside k_analyze); WAVE = full frames are
 * analysed one subframe per wave (k_analyze_w), the partial ones by k_analyze
 * beside it; otherwise every subframe goes to the k_analyze workgroup kernel.  FRA_PLAN_DIRECT_WRITE is never
 * set (the direct-write path was measured slower than slots + k_assemble and removed in r03).  KEEP17 (with
 * WAVE) = the next execute's k_analyze_w keeps residuals up to 17 bits (else 16): a pipelined plan picks the
 * instance from how many waves of an earlier execute needed bit 16 (FRA_KEEP17=0/1 in the environment forces it);
 * both produce the same bytes.
 * The load paths of the next execute, for the plan's strides, windows and current raster pointer (a host raster is
 * copied to a hipMalloc'ed, 256-byte aligned buffer): LOAD_VEC8 = the analysis kernels load samples as 8-byte
 * vectors (else element by element); MINMAX_VEC16 / MINMAX_VEC8 = the min/max pass loads 16- / 8-byte vectors
 * (neither: element by element, also when norm == 0 and nothing is reduced); OFF32 = every frame's rows of one
 * channel span less than 2^31 bytes, so the vector loads may use 32-bit lane offsets (else 64-bit addresses; WAVE
 * needs LOAD_VEC8 and OFF32).  Every combination produces the same bytes. */
#define FRA_PLAN_DIRECT_WRITE 1
#define FRA_PLAN_PIPELINED 2
#define FRA_PLAN_WAVE 4
#define FRA_PLAN_KEEP17 8
#define FRA_PLAN_LOAD_VEC8 16
#define FRA_PLAN_MINMAX_VEC16 32
#define FRA_PLAN_MINMAX_VEC8 64
#define FRA_PLAN_OFF32 128
FRA_API int fra_plan_flags(fra_plan *plan, int32_t *flags);

/* page-locked host memory (hipHostMalloc / hipHostRegister, portable across devices) */
FRA_API int fra_host_alloc(uint64_t bytes, void **host_ptr);
FRA_API int fra_host_free(void *host_ptr);
FRA_API int fra_host_register(void *host_ptr, uint64_t bytes);
FRA_API int fra_host_unregister(void *host_ptr);

/* One-shot convenience: plan, execute, download.  *out (malloc'ed, fra_free) receives the
 * concatenated frames; infos must hold job->nwindows entries. */
FRA_API int fra_encode(int device, const fra_job *job, uint8_t **out, uint64_t *out_len, fra_stream_info *infos);

/* fLaC + STREAMINFO(min=max blocksize, sizes 0, total samples 0, MD5 0) + VORBIS_COMMENT(vendor,
 * 0 comments, last) -- the 86-byte libFLAC 1.4.3 stream header layout. */
FRA_API int fra_stream_header(uint8_t *out86, int32_t channels, int32_t bps, int32_t sample_rate, int32_t blocksize);

/* normalize_to_audio (normalization.py:126-202) on the GPU for n elements of any dtype:
 * mn = nanmin, mx = nanmax unless overridden (data_min / data_max non-NULL), R = mx - mn or 1.0 if
 * mx <= mn, y = ((2.0*(x-mn))/R) - 1.0, clip[-1,1], NaN -> 0, then *32767 -> int16 (bps 16),
 * *8388607 -> int32 (bps 24), *2147483647 -> int32 (any other bps), truncating.
 * data: host or device (on_device) pointer; out_host: host buffer of n int16/int32.
 * mn_out/mx_out receive the (possibly NaN) min/max actually used. */
FRA_API int fra_normalize(fra_ctx *ctx, const void *data, int32_t on_device, int32_t dtype, uint64_t n, int32_t bps,
                          const double *data_min, const double *data_max, void *out_host, double *mn_out,
                          double *mx_out);

/* Native FLAC decoder (read side; replaces pyflac.FileDecoder at
 * converter.py:179-183): frame-parallel host decode of a complete stream (ID3v2 prefix allowed).
 * *samples (malloc'ed, fra_free) receives nsamples x channels interleaved int32.  With
 * FRA_DECODE_CONCAT, streams concatenated after the first one (the --spatial file layout,
 * spatial_encoder.py:196-245) are appended if their format matches. Every CRC-8/CRC-16 is
 * verified; a corrupt or truncated frame fails with FRA_E_INVALID. */
#define FRA_DECODE_CONCAT 1
typedef struct {
  int32_t sample_rate, channels, bps, blocksize; /* STREAMINFO (blocksize = max blocksize) */
  int64_t nframes;
  uint64_t nsamples;                             /* per channel */
  int32_t nstreams;
  uint64_t audio_offset;                         /* first frame byte of the first stream */
} fra_decoded;
FRA_API int fra_decode(const uint8_t *data, uint64_t len, int32_t flags, fra_decoded *info, int32_t **samples);

/* Batched FLAC decode on the GPU: tile streams -> raster (the inverse of the fused normalise + encode path).
 * Every item is one FLAC stream inside `data` whose samples fill one window of the destination: sample p of
 * channel c lands at element c*band_stride + (row_off + p / width)*row_stride + (col_off + p % width)*col_stride
 * of dst.  Without frame_offsets the host lists the sync candidates (header CRC-8) of each stream and the GPU
 * decodes and CRC-16-checks every candidate (k_dec_parse); the frames are chained exactly as in fra_decode.
 * With frame_offsets (a plan's own output: fra_plan_frame_offsets + fra_plan_device_output) nothing is searched
 * and the input may stay on the device.  The frames are then restored (k_dec_restore) and scattered
 * (k_dec_scatter: wasted bits, stereo undo, optional denormalisation, placement).
 *   FRA_DENORM_NONE   dst_dtype FRA_I16 (streams of <= 16 bps only) or FRA_I32: the integers fra_decode returns.
 *   FRA_DENORM_INT    denormalize_from_audio on the exact integers (normalization.py:205-253): y = s / scale
 *                     (32767 for <= 16 bps, else 8388607), x = (y + 1.0) / 2.0 * (data_max - data_min) + data_min,
 *                     integer dst: round half even, float dst: cast; every step a separate IEEE f64 operation.
 *   FRA_DENORM_PCM16  flac_to_tiff's result (F8): y = s / 32768.0 (<= 16 bps) or (s >> 16) / 32768.0, same map.
 * Float -> integer conversions outside the destination type's range saturate (NaN -> 0); numpy leaves them
 * undefined.  What the device path does not cover -- a side channel of a 32-bps stream (33-bit samples), a
 * window of more than 2^31 - 1 samples -- fails with FRA_E_INVALID and a message saying it is not supported on
 * the device; it is never decoded differently from fra_decode.  A corrupt or truncated frame fails with
 * FRA_E_INVALID ("lost sync / corrupt frame at byte N", N relative to the item).  Scratch is allocated per call
 * and freed on every path; on failure dst may be partly written.  dst on the host is copied back before return
 * and must then be one allocation spanning every addressed element from element 0. */
#define FRA_DENORM_NONE 0
#define FRA_DENORM_INT 1
#define FRA_DENORM_PCM16 2
typedef struct {
  uint64_t offset, bytes;        /* one FLAC stream (fLaC ... last frame; ID3v2 prefix allowed) inside data */
  fra_window window;             /* destination of its samples; height*width == samples per channel.  A caller
                                    that does not know the count passes width 1 and height = -capacity: up to
                                    capacity samples are written one per row and infos[i].nsamples reports the
                                    count; more than capacity fails with FRA_E_SPACE before anything is written,
                                    with the needed count in infos[i].nsamples */
  double data_min, data_max;     /* for denormalisation; ignored when denorm == FRA_DENORM_NONE */
  const uint64_t *frame_offsets; /* optional: nframes+1 offsets relative to `offset`, frames only (no header):
                                    skips candidate search and chain; sample_rate/bps/channels/blocksize
                                    then come from the fields below */
  int32_t nframes, channels, bps, blocksize;
} fra_decode_item;

typedef struct {
  const uint8_t *data; uint64_t len; int32_t data_on_device;
  const fra_decode_item *items; int32_t nitems;
  int32_t flags;                 /* FRA_DECODE_CONCAT */
  void *dst; int32_t dst_on_device;
  int32_t dst_dtype;             /* fra_dtype */
  int32_t denorm;                /* FRA_DENORM_NONE | FRA_DENORM_INT | FRA_DENORM_PCM16 */
  int32_t channels; int64_t band_stride, row_stride, col_stride;
} fra_decode_job;

FRA_API int fra_decode_device(fra_ctx *ctx, const fra_decode_job *job, fra_decoded *infos /* nitems */);

/* Windowed read: the pixels of `roi` only, bit-identical to cropping what fra_decode_device gives.  items[i].window
 * is the tile's window in source-raster coordinates (as a streaming container's index gives it) and roi is in the
 * same coordinates (height > 0, width > 0, origin >= 0).  dst is addressed relative to the region: raster pixel
 * (R, C) of channel ch inside both roi and items[i].window lands at element ch*band_stride + (R - roi.row_off)*row_stride
 * + (C - roi.col_off)*col_stride; no other element is written (a host dst keeps the caller's values there).
 * Denormalisation, destination dtypes and saturation are those of fra_decode_device.
 *   An item that does not intersect roi is validated (it must lie inside data) but its bytes are never read; its
 * infos[i] has nframes == 0 and nsamples == 0.  For an intersecting item infos[i].nframes is the number of frames
 * decoded and nsamples the number of pixels of the intersection.
 *   For a tile (r0, c0, H, W) with intersection rows [ra, rb) and columns [ca, cb) the needed samples are
 * [p_lo, p_hi), p_lo = (ra-r0)*W + (ca-c0), p_hi = (rb-1-r0)*W + (cb-c0), and the needed frames p_lo / blocksize
 * through (p_hi-1) / blocksize: only those are parsed, restored and scattered, and scratch and every table are
 * sized by them.  With frame_offsets, frame f is entry f and starts at sample f * blocksize (header numbers are not
 * consulted).  Without, the host keeps the sync candidates whose header frame number lies in that range and chains
 * them locally (from the first audio byte for frame 0, else from each candidate carrying the first number, in byte
 * order; the first chain of consecutive numbers with valid CRC-16s wins).  Every selected frame must have a valid
 * CRC-16, follow its predecessor byte for byte and, unless it is the stream's last, hold blocksize samples, and
 * the last one must reach p_hi: otherwise FRA_E_INVALID ("lost sync / corrupt frame at byte N", N relative to the
 * item, or "the stream ends before the window").
 *   Accepted limitation: damage in a frame that was not selected is not detected -- the price of not reading it.
 *   Refused with FRA_E_INVALID: FRA_DECODE_CONCAT, the capacity form height < 0, a stream whose STREAMINFO minimum
 * and maximum block sizes differ or whose frames carry the variable-blocksize flag, and 33-bit samples. */
FRA_API int fra_decode_device_window(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                     fra_decoded *infos /* nitems */);
/* HIP-event times of the calling thread's last successful fra_decode_device or fra_decode_device_window:
 * 0 k_dec_parse, 1 k_dec_restore, 2 k_dec_scatter, 3 first kernel to last (includes the frame-table copy and the
 * host chain) */
FRA_API int fra_decode_device_timing(float *ms4);

/* Decimated reads: a raster, or a region of a set of tile streams, at 1/factor resolution, factor one of 2, 4, 8, 16,
 * 32, 64 (k below).  The h x w input is cut into k x k blocks anchored at its origin: block (R, C) covers rows
 * [R k, min(R k + k, h)) and columns [C k, min(C k + k, w)) and holds n = rows x columns pixels (edge blocks are
 * smaller).  The output is (channels, oh, ow), oh = ceil(h / k), ow = ceil(w / k), in the input's dtype.
 *   FRA_RESAMPLE_NEAREST  out[b, R, C] = in[b, min(R k + k/2, h - 1), min(C k + k/2, w - 1)]
 *   FRA_RESAMPLE_AVERAGE  integer dtypes: S = the exact integer sum of the block (|S| < 2^44),
 *                         out = rint((double)S / (double)n), round half to even; no summation order is implied.
 *                         f32 / f64: every element is converted to f64; each block row is padded with +0.0 to k elements
 *                         and summed by the adjacent-pair tree ((x0 + x1), (x2 + x3), ... then pairs of those, log2 k
 *                         levels); the row sums are accumulated top to bottom (acc = row 0; acc += row 1; ...; rows the
 *                         block does not have are not added); out = (T)(acc / (double)n).  Plain IEEE arithmetic: NaN
 *                         and +-inf propagate, nothing is skipped.
 * With a geotransform (a, b, c, d, e, f) and the input's origin at (row, col) the output's transform is
 * (a k, b k, c + col a + row b, d k, e k, f + col d + row e). */
#define FRA_RESAMPLE_NEAREST 0
#define FRA_RESAMPLE_AVERAGE 1
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype, of src and dst */
  int32_t channels, height, width;          /* >= 1 */
  int64_t src_band_stride, src_row_stride, src_col_stride;  /* elements, >= 0 */
  int32_t factor, resampling;
  void *dst; int32_t dst_on_device;         /* (channels, oh, ow) through the strides below */
  int64_t dst_band_stride, dst_row_stride, dst_col_stride;
} fra_decimate_job;
/* k_decimate alone, over a host or device raster of any dtype.  Synchronous.  Host buffers are staged as the decoder
 * stages them: each must be one allocation spanning every addressed element from element 0; the elements of dst that
 * are not outputs keep the caller's values.  Rows are read with 16-byte loads when src_col_stride == 1 and src, the row
 * stride and the band stride are multiples of 16 bytes, element by element otherwise (any layout, e.g. pixel-interleaved).
 * FRA_E_INVALID, before any GPU work, for a null argument, a factor outside the six values, an unknown resampling code,
 * a bad dtype or layout. */
FRA_API int fra_decimate(fra_ctx *ctx, const fra_decimate_job *job);
/* The windowed read at 1/factor resolution: exactly the decimation (rule above) of what fra_decode_device_window would
 * have written for `roi`, in dst_dtype, after its denormalisation and saturation.  roi, the items and infos mean what
 * they mean there; the job's dst and strides address the oh x ow output (h = roi->height, w = roi->width), and no other
 * element is written.  The call runs fra_decode_device_window into a per-call device buffer of the region (band-planar,
 * rows padded to 16 bytes), so every refusal and message of the windowed read is this call's as well; then k_decimate on
 * the context's stream; then, for a host dst, the copy back.  The region buffer is released on every path.  Device
 * memory: the windowed read's scratch beside the region buffer, then the region buffer beside a staged host dst.
 *   FRA_E_INVALID before any GPU work: a null argument, a factor outside the six values, an unknown resampling code, and
 * items whose intersections with roi do not add up to roi's area ("the items do not cover the region"): every pixel of
 * the region must be decoded, since an average reads all of them.  Overlapping items remain the caller's contract.
 *   Afterwards fra_decode_device_timing reports the inner windowed read and fra_decimate_timing the decimation. */
FRA_API int fra_decode_device_decimated(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi, int32_t factor,
                                        int32_t resampling, fra_decoded *infos /* nitems */);
/* HIP-event time (ms) of the calling thread's last k_decimate (fra_decimate or fra_decode_device_decimated) */
FRA_API int fra_decimate_timing(float *ms);

/* Resampled reads: a raster, or a region of a set of tile streams, at any output size: (channels, h, w) ->
 * (channels, oh, ow), 1 <= oh, ow <= 65536, larger or smaller than the input, in the input's dtype (any fra_dtype).
 * Each axis is handled alone and the same way (columns below): g = gcd(w, ow), w' = w / g, ow' = ow / g; rows: h', oh'.
 * Every coordinate is an integer (no floating-point coordinate is formed); every value operation is an IEEE f64
 * operation rounded on its own (no contraction).  NaN and +-inf propagate, nothing is skipped, there is no nodata.
 *   The centre of output column C lies at source coordinate (C + 1/2) w / ow - 1/2:
 *     num = (2 C + 1) w' - ow', den = 2 ow', i0 = floor(num / den) (negative for the first columns when upsampling),
 *     t = (double)(num - i0 den) / (double)den, one correctly rounded division of two exact integers.
 *   FRA_RESAMPLE_NEAREST   out[R, C] = in[min(((2 R + 1) h') / (2 oh'), h - 1), min(((2 C + 1) w') / (2 ow'), w - 1)]
 *                          (for k dividing h and w and (oh, ow) = (h / k, w / k): the decimation's nearest)
 *   FRA_RESAMPLE_BILINEAR  taps i0, i0 + 1, weights [1.0 - t, t]
 *   FRA_RESAMPLE_CUBIC     taps i0 - 1 .. i0 + 2 (Catmull-Rom, a = -1/2), weights by exactly these operations:
 *                            ((-0.5 t + 1.0) t - 0.5) t,  ((1.5 t - 2.5) t) t + 1.0,
 *                            ((-1.5 t + 2.0) t + 0.5) t,  ((0.5 t - 0.5) t) t
 *                          Both: every tap index is clamped to [0, w - 1]; vertically first, for every tap column
 *                          c_i = sum_j (double)x[j][i] wy_j top to bottom (acc = p0; acc += p1; ...), then
 *                          v = sum_i c_i wx_i left to right the same way.  f32 / f64: out = (T)v; integer dtypes:
 *                          out = rint(v), half to even, clamped to the dtype's range (cubic overshoots).
 *   FRA_RESAMPLE_AVERAGE   area weights in units of 1 / ow' of a source pixel: output column C covers [C w', (C + 1) w'),
 *                          source column i covers [i ow', (i + 1) ow'); vx_i = min((i + 1) ow', (C + 1) w') -
 *                          max(i ow', C w') for the columns where it is positive (they sum to w'); vy_j likewise;
 *                          n = h' w'.  Integer dtypes: S = sum_j sum_i vy_j vx_i x[j][i], exact in int64 (no summation
 *                          order is implied), out = rint((double)S / (double)n), half to even; FRA_E_INVALID when
 *                          n 2^(8 itemsize) > 2^63.  f32 / f64: c_i = sum_j (double)vy_j (double)x[j][i] top to bottom,
 *                          acc = sum_i (double)vx_i c_i left to right, out = (T)(acc / (double)n); FRA_E_INVALID when
 *                          n > 2^53.  (For k dividing h and w and (oh, ow) = (h / k, w / k) every weight is 1 and the
 *                          integer result is the decimation's average.)
 *   When (oh, ow) = (h, w) every mode returns the input.
 * With a geotransform (a, b, c, d, e, f), the input's origin at (row, col), sx = w / ow and sy = h / oh the output's
 * transform is (a sx, b sy, c + col a + row b, d sx, e sy, f + col d + row e). */
#define FRA_RESAMPLE_BILINEAR 2
#define FRA_RESAMPLE_CUBIC 3
#define FRA_RESAMPLE_MAX_OUT 65536
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype, of src and dst */
  int32_t channels, height, width;          /* >= 1 */
  int64_t src_band_stride, src_row_stride, src_col_stride;  /* elements, >= 0 */
  int32_t out_height, out_width;            /* 1 .. FRA_RESAMPLE_MAX_OUT */
  int32_t resampling;                       /* FRA_RESAMPLE_* (all four) */
  void *dst; int32_t dst_on_device;         /* (channels, out_height, out_width) through the strides below */
  int64_t dst_band_stride, dst_row_stride, dst_col_stride;
} fra_resample_job;
/* k_resample alone, over a host or device raster of any dtype.  Synchronous.  Host buffers are staged as fra_decimate
 * stages them (one allocation spanning every addressed element from element 0; the elements of dst that are not
 * outputs keep the caller's values).  The average reads rows with 16-byte loads when src_col_stride == 1 and src, the
 * row stride and the band stride are multiples of 16 bytes, element by element otherwise.
 * FRA_E_INVALID, before any GPU work, for a null argument, a bad dtype or layout, an output size outside
 * 1 .. 65536, an unknown resampling code and the two overflow bounds of the average. */
FRA_API int fra_resample(fra_ctx *ctx, const fra_resample_job *job);
/* The windowed read at any output size: exactly the resampling (rule above) of what fra_decode_device_window would
 * have written for `roi`, in dst_dtype, after its denormalisation and saturation.  Built as
 * fra_decode_device_decimated is: the windowed read into a per-call device buffer of the region (its refusals and
 * messages are this call's), then k_resample on the context's stream, then, for a host dst, the copy back; the job's
 * dst and strides address the out_height x out_width output and no other element is written.  The region buffer is
 * released on every path.
 *   FRA_E_INVALID before any GPU work: a null argument, an output size outside 1 .. 65536, an unknown resampling code,
 * the overflow bounds of the average, and items that do not cover the region ("the items do not cover the region").
 *   Afterwards fra_decode_device_timing reports the inner windowed read and fra_resample_timing the resampling. */
FRA_API int fra_decode_device_resampled(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                        int32_t out_height, int32_t out_width, int32_t resampling,
                                        fra_decoded *infos /* nitems */);
/* HIP-event time (ms) of the calling thread's last k_resample (fra_resample or fra_decode_device_resampled) */
FRA_API int fra_resample_timing(float *ms);

/* Nodata-aware reads: the resampling and the decimation above with one value, and NaN, left out of every result.
 *
 * A nodata value nd is a double.
 *   For integer dtypes nd must be an integer inside the dtype's range.
 *   For float32 / float64 nd must be NaN, or finite and exactly representable in the dtype.
 *   Anything else is refused before any GPU work: ValueError in Python, FRA_E_INVALID in the C ABI.  An infinite nd
 *   is refused too.
 *   A pixel x is invalid when (double)x == nd, the same test as the statistics.  In float dtypes a NaN pixel is also
 *   invalid, whatever nd is.  +-inf are valid and propagate by IEEE arithmetic.  The fill is (T)nd.
 * Coordinates, taps, weights, g, h', w', i0 and t are exactly those of the unmasked rule.  Only the value arithmetic
 * below is new.  Every f64 operation is rounded on its own.
 *   nearest   unchanged: it picks one pixel, invalid or not.
 *   average   (resample)  Down the output row's source rows j, top to bottom, for every source column i:
 *             integer dtypes: c_i = the sum of vy_j x[j][i] over the valid pixels, exact in int64; float dtypes: the
 *             first valid term initialises c_i and later valid terms are added (c_i = term; c_i += term; ...).
 *             u_i = the integer sum of vy_j over the valid pixels.
 *             Then over the output's source columns i, left to right, skipping the columns with u_i == 0:
 *             S = sum_i vx_i c_i (floats: acc = (double)vx_i * c_i, the first non-skipped column initialising) and
 *             W = sum_i vx_i u_i, exact in int64, 1 <= W <= n.  W == 0 gives the fill.  Otherwise integers give
 *             rint((double)S / (double)W), half to even (between the valid extremes: no clamp), and floats give
 *             (T)(acc / (double)W).  The two overflow bounds of the unmasked average apply unchanged.
 *             With no invalid pixel the result equals the unmasked resampling bit for bit in every dtype, -0.0
 *             included.  An average of valid pixels that happens to land on nd is written as it is (possible only
 *             when nd lies strictly inside the data's range); nothing is nudged.
 *   average   (decimate, factor k)  The same arithmetic with h' = w' = k and oh' = ow' = 1: every weight is 1, the tap
 *             ranges are clipped at the raster's edge, the output is ceil(h / k) x ceil(w / k), and edge blocks need
 *             no special case because the divisor is W, the count of valid pixels.  The float summation order is the
 *             one above, not the adjacent-pair tree of the unmasked decimation.  So for k dividing h and w the
 *             decimation equals the resampling to (h / k, w / k) bit for bit in every dtype, and with no invalid
 *             pixel it equals the unmasked decimation for integer dtypes only.
 *   bilinear, cubic   If all taps of the output (4 or 16, after clamping) are valid, the result is the unmasked
 *             formula exactly, with no division.  Otherwise the result is the masked bilinear of the same centre,
 *             whichever of the two modes was asked for (a cubic kernel's negative weights cannot be renormalised
 *             safely): taps i0, i0 + 1 per axis, clamped, weights wy = [1.0 - ty, ty] and wx likewise.  Vertically
 *             c_i = the sum of (double)x[j][i] * wy_j over the valid j in ascending order, the first valid term
 *             initialising, and u_i = the sum of wy_j over the valid j.  Horizontally, over the columns with at
 *             least one valid tap, v = sum_i c_i * wx_i and Wt = sum_i u_i * wx_i in ascending order, the first such
 *             column initialising both.  No valid tap, or Wt <= 0.0 (a lone valid tap with weight exactly 0), gives
 *             the fill.  Otherwise q = v / Wt; floats give (T)q, integers rint(q) clamped to the dtype.
 *   When (oh, ow) = (h, w) every mode of the resampling returns the input.
 *
 * filled (host memory, `channels` words, may be NULL) receives per band the number of output pixels that no valid pixel
 * reached: those written as the fill by the average, the bilinear and the cubic; for the nearest and for an output of
 * the input's size, the picked pixels that are invalid.  The kernel adds them up within each wave and issues one
 * atomicAdd per workgroup into a zeroed device array. */
/* fra_resample with a nodata value (rule above).  Buffers, layouts and refusals as fra_resample; also FRA_E_INVALID,
 * before any GPU work, for a nodata value the dtype does not admit. */
FRA_API int fra_resample_masked(fra_ctx *ctx, const fra_resample_job *job, double nodata,
                                uint64_t *filled /* channels, may be NULL */);
/* fra_decimate with a nodata value (rule above).  Buffers, layouts and refusals as fra_decimate; also FRA_E_INVALID,
 * before any GPU work, for a nodata value the dtype does not admit. */
FRA_API int fra_decimate_masked(fra_ctx *ctx, const fra_decimate_job *job, double nodata,
                                uint64_t *filled /* channels, may be NULL */);
/* fra_decode_device_resampled with a nodata value: the windowed read into a per-call device buffer of the region (its
 * refusals and messages are this call's), then k_resample_masked, then, for a host dst, the copy back.  The region buffer
 * is released on every path.  FRA_E_INVALID before any GPU work for everything fra_decode_device_resampled refuses so,
 * and for a nodata value that dst_dtype does not admit. */
FRA_API int fra_decode_device_resampled_masked(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                               int32_t out_height, int32_t out_width, int32_t resampling,
                                               fra_decoded *infos /* nitems */, double nodata,
                                               uint64_t *filled /* channels, may be NULL */);
/* fra_decode_device_decimated with a nodata value, built the same way.  FRA_E_INVALID before any GPU work for everything
 * fra_decode_device_decimated refuses so, and for a nodata value that dst_dtype does not admit. */
FRA_API int fra_decode_device_decimated_masked(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                               int32_t factor, int32_t resampling, fra_decoded *infos /* nitems */,
                                               double nodata, uint64_t *filled /* channels, may be NULL */);
/* HIP-event time (ms) of the calling thread's last k_resample_masked (any of the four entries above) */
FRA_API int fra_resample_masked_timing(float *ms);

/* Comparison of two rasters a and b of one dtype (any fra_dtype) and shape (channels, h, w): one report per band.
 *   Integer dtypes: d = (int64)a - (int64)b, exact, never wrapping (|d| <= 2^32 - 1).  differing = pixels with d != 0;
 *     first_row / first_col = the first of them in row-major order, relative to the rasters' origin (-1, -1: none);
 *     max_abs = max |d| (a double, exact); sum_abs = sum |d| (exact uint64); sum_sq_lo / _hi = sum d^2 as an exact 128-bit
 *     integer; a_min, a_max, b_min, b_max exact doubles; unordered = 0, fsum_abs = fsum_sq = 0.  More than 2^32 pixels per
 *     band are refused (FRA_E_INVALID), which keeps sum_abs inside 64 bits.
 *   f32 / f64: every element is converted to f64.  Both non-NaN: the pixel is equal iff a == b (-0.0 equals +0.0);
 *     d = 0.0 when equal, else a - b (+-inf propagates by plain IEEE arithmetic); |d| goes to max_abs and fsum_abs, d * d to
 *     fsum_sq.  Both NaN: counted in unordered, not in differing, contributes nothing.  Exactly one NaN: counted in
 *     unordered and in differing, eligible for first_*, contributes nothing to max_abs or the sums.  The minima and maxima
 *     skip NaN and are NaN when the band holds no number.  sum_abs = sum_sq_* = 0.  differing == 0 is exactly
 *     numpy.array_equal(a, b, equal_nan=True).
 *     fsum_abs and fsum_sq are f64 sums and no summation order is implied; but no float atomics are used -- each workgroup
 *     reduces by a fixed lane tree to one partial record and a second kernel adds a band's partials in index order -- so two
 *     calls on the same inputs and layout return byte-identical reports.
 *   count = h * w in every report. */
typedef struct {
  uint64_t count, differing, unordered;
  int64_t  first_row, first_col;
  uint64_t sum_abs, sum_sq_lo, sum_sq_hi;
  double   max_abs, fsum_abs, fsum_sq, a_min, a_max, b_min, b_max;
  uint64_t reserved;  /* 0 */
} fra_compare_band;   /* 128 bytes */
typedef struct {
  const void *a; int32_t a_on_device;       /* element (band 0, row 0, col 0); host memory is copied to the device */
  int64_t a_band_stride, a_row_stride, a_col_stride;  /* elements, >= 0 */
  const void *b; int32_t b_on_device;
  int64_t b_band_stride, b_row_stride, b_col_stride;
  int32_t dtype;                            /* fra_dtype, of a and b */
  int32_t channels, height, width;          /* >= 1 */
} fra_compare_job;
/* k_compare + k_compare_fold alone, over host or device rasters.  Synchronous; bands (host memory) receives `channels`
 * reports.  Host rasters are staged as fra_decimate stages them: each must be one allocation spanning every addressed
 * element from element 0.  Neither raster is written.  Both are read with 16-byte loads when, for both, the column stride
 * is 1 and the base, the row stride and the band stride are multiples of 16 bytes; element by element otherwise (any
 * layout, e.g. pixel-interleaved).  FRA_E_INVALID, before any GPU work, for a null argument, a bad dtype, a bad layout
 * (channels, height or width < 1, a negative stride) and more than 2^32 pixels per band. */
FRA_API int fra_compare(fra_ctx *ctx, const fra_compare_job *job, fra_compare_band *bands /* channels */);
/* The windowed read compared with a reference raster, a = what fra_decode_device_window would have written for `roi` (in
 * dst_dtype, after its denormalisation and saturation), b = ref: does this container give that raster back, and if not, by
 * how much.  roi, the items and infos mean what they mean there.  ref (host or device) is addressed relative to the region,
 * in job->dst_dtype: pixel (R, C) of channel ch at ch*ref_band_stride + (R - roi.row_off)*ref_row_stride +
 * (C - roi.col_off)*ref_col_stride; first_row / first_col are relative to the region too.  job->dst, dst_on_device and the
 * job's strides are ignored (they may be null / 0).  The call runs fra_decode_device_window into a per-call device buffer
 * of the region (band-planar, rows padded to 16 bytes), so every refusal and message of the windowed read is this call's as
 * well; then k_compare of that buffer against ref on the context's stream.  The decoded region never leaves the device and
 * its buffer is released on every path.  Device memory: the windowed read's scratch beside the region buffer, then the
 * region buffer beside a staged host ref.
 *   FRA_E_INVALID before any GPU work: a null argument (ref and bands included), a negative ref stride, more than 2^32
 * pixels, and items whose intersections with roi do not add up to roi's area ("the items do not cover the region"): every
 * pixel of the region must be decoded, since every one is compared.  Overlapping items remain the caller's contract.
 *   Afterwards fra_decode_device_timing reports the inner windowed read and fra_compare_timing the comparison. */
FRA_API int fra_decode_device_compare(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi, const void *ref,
                                      int32_t ref_on_device, int64_t ref_band_stride, int64_t ref_row_stride,
                                      int64_t ref_col_stride, fra_compare_band *bands /* channels */,
                                      fra_decoded *infos /* nitems */);
/* HIP-event time (ms) of the calling thread's last k_compare + k_compare_fold (fra_compare or fra_decode_device_compare) */
FRA_API int fra_compare_timing(float *ms);

/* Band statistics and histograms of a raster (channels, h, w) of any fra_dtype: one report per band.
 *   Which pixels count.  Every element is taken as f64 (exact for all eight dtypes).  nan = the NaN pixels (floats only);
 *     nodata = the pixels with (double)x == opts.nodata, counted only with FRA_STATS_NODATA (a NaN nodata matches
 *     nothing); valid = the rest, and only valid pixels enter anything below.  count = h * w = valid + nan + nodata.
 *     +-inf are valid numbers.
 *   Extremes.  min, max over the valid pixels, exact doubles, +-inf included; NaN when valid == 0.  fin_min, fin_max the
 *     same over the finite valid pixels, NaN when there is none; for integers they equal min / max.
 *   Integer dtypes.  sum = the exact 128-bit two's-complement sum of x (sum_lo uint64, sum_hi int64); sq = the exact
 *     unsigned 128-bit sum of x^2 (sq_lo, sq_hi).  No order is implied, nothing wraps.  More than 2^32 pixels per band are
 *     refused, which keeps sum inside 65 bits and sq inside 96.  fsum = mean = fm2 = 0.0.
 *   f32 / f64.  fsum = the f64 sum of x; mean = fsum / (double)valid, one IEEE division; fm2 = the f64 sum of
 *     (x - mean) * (x - mean), the corrected two-pass form with mean read back from the first pass on the device.  No
 *     summation order is implied, but no float atomics are used -- lane tree, then the waves in order, then the partials in
 *     index order -- so two calls on the same inputs and layout return byte-identical reports.  Plain IEEE arithmetic:
 *     +-inf propagate into fsum, mean and fm2, which may become inf or NaN.  valid == 0: fsum = fm2 = 0.0, mean = NaN.
 *     The integer sums are 0.
 *   Histogram.  opts.bins in 0 ... 65536, 0 = none; hist is channels x bins uint64, zero where nothing falls.  The range of
 *     a band is [opts.hist_lo, opts.hist_hi] (both finite, lo <= hi), or with FRA_STATS_AUTO_RANGE [fin_min, fin_max] of
 *     that band, read on the device from the first pass.  scale = hi > lo ? (double)bins / (hi - lo) : 0.0, and a scale
 *     that is not finite is taken as 0.0.  A valid pixel with x < lo goes to below, one with x > hi to above, any other
 *     to bin min(bins - 1, (int64)floor((x - lo) * scale)) (bin 0 when scale == 0.0): the subtraction, the product and
 *     the floor are separate f64 operations.  A band without an automatic range (no finite valid pixel) bins nothing and
 *     has below = above = 0.  hist_lo, hist_hi, hist_scale are the values used: 0 when bins == 0, NaN / NaN / 0 for a band
 *     without a range.  When hi - lo == bins the scale is exactly 1.0 and bin i holds exactly the pixels of value lo + i:
 *     uint16 over [0, 65536] with 65536 bins is the exact value histogram, and so for every dtype of <= 16 bits. */
#define FRA_STATS_AUTO_RANGE 1
#define FRA_STATS_NODATA 2
typedef struct {
  int32_t bins, flags;
  double hist_lo, hist_hi, nodata;
} fra_stats_opts;
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype */
  int32_t channels, height, width;          /* >= 1 */
  int64_t band_stride, row_stride, col_stride;  /* elements, >= 0 */
  fra_stats_opts opts;
} fra_stats_job;
typedef struct {
  uint64_t count, valid, nan, nodata, below, above;
  uint64_t sum_lo; int64_t sum_hi; uint64_t sq_lo, sq_hi;
  double   min, max, fin_min, fin_max, fsum, mean, fm2, hist_lo, hist_hi, hist_scale;
} fra_stats_band;     /* 160 bytes */
/* k_stats + its fold (and, for floats and for an automatic range, the second pass + its fold) alone, over a host or
 * device raster of any layout.  Synchronous; bands (host memory) receives `channels` reports and hist (host memory)
 * channels x bins counts; hist may be null only when bins == 0.  A host raster is staged as fra_compare stages it (one
 * allocation spanning every addressed element from element 0) and never written; 16-byte loads when the column stride
 * is 1 and the base, the row stride and the band stride are multiples of 16 bytes, element loads otherwise.
 * FRA_E_INVALID, before any GPU work: a null argument, a bad dtype or layout, more than 2^32 pixels per band, bins
 * outside 0 ... 65536, unknown flag bits, a non-finite or inverted explicit range, a null hist with bins > 0. */
FRA_API int fra_stats(fra_ctx *ctx, const fra_stats_job *job, fra_stats_band *bands /* channels */,
                      uint64_t *hist /* channels x bins */);
/* The statistics of what fra_decode_device_window would have written for `roi`, in dst_dtype, after its
 * denormalisation and saturation.  roi, the items and infos mean what they mean there; job->dst and the job's strides
 * are ignored.  The region goes to a per-call device buffer (band-planar, rows padded to 16 bytes) and never leaves the
 * device; every refusal and message of the windowed read is this call's as well, items that do not cover the region are
 * refused as by fra_decode_device_compare, and the options as by fra_stats.  Afterwards fra_decode_device_timing
 * reports the inner windowed read and fra_stats_timing the statistics. */
FRA_API int fra_decode_device_stats(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                    const fra_stats_opts *opts, fra_stats_band *bands /* channels */,
                                    uint64_t *hist /* channels x bins */, fra_decoded *infos /* nitems */);
/* HIP-event time (ms) of the calling thread's last statistics kernels, both passes and folds */
FRA_API int fra_stats_timing(float *ms);

/* Band math: per-pixel expressions over the bands of a raster (channels, h, w) of any fra_dtype, one expression per
 * output band of a raster (nout, h, w) of any fra_dtype.  This unit maps a raster; the five above reduce one.
 *   The program.  A stack program in reverse Polish notation, code[i] = op | arg << 8, at most FRA_CALC_MAX_CODE words,
 *     FRA_CALC_MAX_CONST f64 constants, FRA_CALC_MAX_OUT outputs and a stack of FRA_CALC_MAX_DEPTH values.  Every value
 *     is an f64; every element of the source is taken as f64 (exact for all eight dtypes).  arg is 0 for every op
 *     without one.
 *       FRA_CALC_CONST k   push consts[k]              FRA_CALC_BAND b   push the pixel's element of band b (0-based)
 *       FRA_CALC_STORE k   pop x: output band k of the pixel is x, converted as below
 *       ADD SUB MUL DIV    pop b, pop a, push a op b   NEG ABS SQRT FLOOR   pop x, push op x
 *       MIN  a < b ? a : b         MAX  a > b ? a : b  (the < / > form, not minNum: MIN(NaN, 1) = 1, MIN(1, NaN) = NaN)
 *       LT LE GT GE EQ NE  pop b, pop a, push 1.0 when a op b holds, else 0.0 (IEEE comparisons: NaN != NaN holds only)
 *       AND OR             pop b, pop a, push 1.0 / 0.0 of the truths of a and b; NOT  pop x, push 1.0 when x is false
 *       SELECT             pop b, pop a, pop c, push c true ? a : b
 *     A value is true when x != 0.0, so NaN is true.  Every op is one IEEE f64 operation rounded on its own: no
 *     contraction, no reassociation, division and square root correctly rounded.  NaN and +-inf flow through as IEEE
 *     gives them.
 *   Output.  f64 / f32: a NaN result becomes the quiet NaN 0x7ff8000000000000 (the sign and payload of a NaN are not
 *     IEEE's to fix), then a plain cast.  Integer dtypes: rint(x), half to even, saturated to the dtype's range, NaN -> 0
 *     (the rule of FRA_DENORM_INT).
 *   Nodata.  With FRA_CALC_NODATA a pixel is left out when any band the program reads (a FRA_CALC_BAND word names it)
 *     holds (double)x == nodata, or NaN; bands the program does not read are not looked at, and a NaN nodata matches
 *     nothing.  Every output band of a left-out pixel gets `fill`, converted as above.  Without the flag nothing is
 *     masked.  left_out receives per output band the number of left-out pixels (one number, nout times).
 *   A program is valid when: 1 <= ncode <= 128, 0 <= nconst <= 32, 1 <= nout <= 8, no unknown flag bit, 1 <= channels
 *     <= 255; every op is known and an op without an argument has arg 0; BAND's arg < channels, CONST's < nconst,
 *     STORE's < nout; the stack never underflows nor exceeds 8 values and is empty after the last word; every output is
 *     stored exactly once.  Any double -- NaN, inf -- is accepted as a constant, as nodata and as fill. */
#define FRA_CALC_MAX_CODE 128
#define FRA_CALC_MAX_CONST 32
#define FRA_CALC_MAX_OUT 8
#define FRA_CALC_MAX_DEPTH 8
#define FRA_CALC_NODATA 1
typedef enum {
  FRA_CALC_CONST = 0, FRA_CALC_BAND = 1, FRA_CALC_STORE = 2,
  FRA_CALC_ADD = 3, FRA_CALC_SUB = 4, FRA_CALC_MUL = 5, FRA_CALC_DIV = 6,
  FRA_CALC_NEG = 7, FRA_CALC_ABS = 8, FRA_CALC_SQRT = 9, FRA_CALC_FLOOR = 10,
  FRA_CALC_MIN = 11, FRA_CALC_MAX = 12,
  FRA_CALC_LT = 13, FRA_CALC_LE = 14, FRA_CALC_GT = 15, FRA_CALC_GE = 16, FRA_CALC_EQ = 17, FRA_CALC_NE = 18,
  FRA_CALC_AND = 19, FRA_CALC_OR = 20, FRA_CALC_NOT = 21, FRA_CALC_SELECT = 22
} fra_calc_op;
typedef struct {
  int32_t ncode, nconst, nout, flags;       /* flags: FRA_CALC_NODATA */
  double nodata, fill;
  uint16_t code[FRA_CALC_MAX_CODE];
  double consts[FRA_CALC_MAX_CONST];
} fra_calc_program;                         /* 544 bytes */
typedef struct {
  void *dst; int32_t dst_on_device;         /* element (band 0, row 0, col 0) of the (nout, h, w) output */
  int32_t dtype;                            /* fra_dtype of the output */
  int64_t band_stride, row_stride, col_stride;  /* elements, >= 0 */
} fra_calc_dst;
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype of the source */
  int32_t channels, height, width;          /* >= 1; channels <= 255 */
  int64_t band_stride, row_stride, col_stride;  /* elements, >= 0 */
  fra_calc_program program;
  fra_calc_dst out;
} fra_calc_job;
/* Whether `program` is valid for a source of `channels` bands (the list above).  Pure host code: no context, no GPU.
 * FRA_E_INVALID with a message that names the offending word ("word 5: ...") or count. */
FRA_API int fra_calc_check(const fra_calc_program *program, int32_t channels);
/* k_calc alone, over a host or device raster of any layout into a host or device raster of any layout.  Synchronous.
 * Host buffers are staged as fra_decimate stages them (one allocation spanning every addressed element from element 0;
 * the elements of dst that are not outputs keep the caller's values).  Rows are read, and written, with vector accesses
 * when the column stride is 1 and the base, the row stride and the band stride are multiples of 16 bytes, element by
 * element otherwise; source and destination are judged separately.  left_out (host memory, nout words, may be NULL).
 * FRA_E_INVALID, before any GPU work and in this order: a null argument, an invalid program (fra_calc_check), a bad
 * source or destination dtype or layout, more than 2^32 pixels per band.  The kernel interprets the program, so nothing
 * is launched for a program that has not passed the check. */
FRA_API int fra_calc(fra_ctx *ctx, const fra_calc_job *job, uint64_t *left_out /* nout, may be NULL */);
/* The program over what fra_decode_device_window would have written for `roi`, in job->dst_dtype, after its
 * denormalisation and saturation.  roi, the items and infos mean what they mean there; job->dst and the job's strides
 * are ignored: the region goes to a per-call device buffer (band-planar, rows padded to 16 bytes) and never leaves the
 * device, and the result goes to `out`, a (program->nout, roi->height, roi->width) raster of out->dtype.  Every refusal
 * and message of the windowed read is this call's as well; items that do not cover the region are refused as by
 * fra_decode_device_compare; the program and `out` as by fra_calc.  Afterwards fra_decode_device_timing reports the
 * inner windowed read and fra_calc_timing the map. */
FRA_API int fra_decode_device_calc(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                   const fra_calc_program *program, const fra_calc_dst *out,
                                   uint64_t *left_out /* nout, may be NULL */, fra_decoded *infos /* nitems */);
/* HIP-event time (ms) of the calling thread's last k_calc (fra_calc or fra_decode_device_calc) */
FRA_API int fra_calc_timing(float *ms);

/* Focal operations: every band of a raster (channels, h, w) of any fra_dtype on its own, a window of kh x kw pixels
 * around each pixel, into a raster (channels, out_h, out_w) of any fra_dtype.  The result covers an output rectangle
 * (row_off, col_off, out_h, out_w) inside the source; neighbours inside the source but outside the rectangle are read,
 * so a rectangle of the result is the crop of the whole-raster result.  This unit maps a raster, like the band math.
 *   Values.  Every value is an f64; every element of the source is taken as f64 (exact for all eight dtypes).  Every
 *     arithmetic step is one IEEE f64 operation rounded on its own: no contraction, no reassociation, division and
 *     square root correctly rounded.  A result is converted as the band math converts one (Output, above).
 *   Window.  kh x kw, both odd, 1 ... 15, centred on the pixel.  Taps are visited in row-major order.
 *   A tap is left out when it is NaN; when FRA_FOCAL_NODATA is set and (double)x == nodata (a NaN nodata matches
 *     nothing); when it lies outside the source and edge is FRA_FOCAL_EDGE_SKIP.  With FRA_FOCAL_EDGE_CLAMP a tap outside
 *     the source is the nearest source pixel (coordinates clamped per axis), left out when that pixel is.  The other
 *     taps are the valid ones; n is their number.
 *   Ops.
 *     SUM       the valid taps added in tap order, starting from the first valid one.
 *     MEAN      that sum / (double)n.
 *     MIN, MAX  m = the first valid tap, then m = x < m ? x : m (MAX: x > m) in tap order.
 *     COUNT     (double)n.
 *     MEDIAN    the lower median, no averaging: the valid taps ordered by value, equal values (-0.0 == 0.0) by tap
 *               order; the one of rank (n - 1) / 2.  kh * kw <= 25.
 *     CONVOLVE  acc = the products (double)x * weights[tap], each rounded, added in tap order starting from the first
 *               valid one; weights is row-major, any double.  With FRA_FOCAL_NORMALIZE the result is acc / ws, ws the
 *               valid taps' weights added the same way; ws == 0.0 gives fill.
 *     SLOPE, HILLSHADE  3 x 3 only, Horn's gradient; the taps are a b c / d e f / g h i, row 0 to the north.
 *               zx = ((c + (f + f)) + i) - ((a + (d + d)) + g),  zy = ((a + (b + b)) + c) - ((g + (h + h)) + i),
 *               p = zx * params[0], q = zy * params[1]; the caller passes params[0] = zfactor / (8 dx) and params[1] =
 *               zfactor / (8 dy).  SLOPE = sqrt(p * p + q * q) * params[2] (1: rise / run, 100: percent).  HILLSHADE,
 *               with the light vector (lx, ly, lz) = params[2 .. 4] (east, north, up): s = ((lz - p * lx) - q * ly) /
 *               sqrt((1.0 + p * p) + q * q), s = s > 0 ? s : 0, result = s * params[5].  No trigonometry: the caller
 *               turns azimuth and altitude into the light vector.  Any of the nine taps left out: fill.
 *   Fill.  A pixel gets `fill` when no tap is valid (COUNT gives 0 instead), when an op above says so, and, with
 *     FRA_FOCAL_KEEP_MASK, when the centre pixel itself is left out.  left_out receives per band the number of output
 *     pixels that got fill.
 *   A spec is valid when: the op, the edge mode and every flag bit are known; kh and kw are odd and in 1 ... 15; MEDIAN
 *     has at most 25 taps; SLOPE and HILLSHADE have a 3 x 3 window; FRA_FOCAL_NORMALIZE comes with CONVOLVE alone.  Any
 *     double is accepted as a weight, a parameter, nodata and fill. */
#define FRA_FOCAL_MAX_SIZE 15
#define FRA_FOCAL_MAX_MEDIAN 25
#define FRA_FOCAL_NODATA 1
#define FRA_FOCAL_NORMALIZE 2
#define FRA_FOCAL_KEEP_MASK 4
typedef enum {
  FRA_FOCAL_SUM = 0, FRA_FOCAL_MEAN = 1, FRA_FOCAL_MIN = 2, FRA_FOCAL_MAX = 3, FRA_FOCAL_COUNT = 4,
  FRA_FOCAL_MEDIAN = 5, FRA_FOCAL_CONVOLVE = 6, FRA_FOCAL_SLOPE = 7, FRA_FOCAL_HILLSHADE = 8
} fra_focal_op;
typedef enum { FRA_FOCAL_EDGE_SKIP = 0, FRA_FOCAL_EDGE_CLAMP = 1 } fra_focal_edge;
typedef struct {
  int32_t op, kh, kw, edge, flags;          /* fra_focal_op, the window, fra_focal_edge, FRA_FOCAL_* flags */
  double nodata, fill;
  double params[8];                         /* SLOPE, HILLSHADE */
  double weights[225];                      /* CONVOLVE: kh * kw, row-major */
} fra_focal_spec;                           /* 1904 bytes */
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype of the source */
  int32_t channels, height, width;          /* >= 1; channels <= 255 */
  int64_t band_stride, row_stride, col_stride;  /* elements, >= 0 */
  fra_window rect;                          /* the output rectangle, inside the source */
  fra_focal_spec spec;
  fra_calc_dst out;                         /* the (channels, rect.height, rect.width) output */
} fra_focal_job;
/* Whether `spec` is valid (the list above).  Pure host code: no context, no GPU.  FRA_E_INVALID with a message that
 * names the offending field. */
FRA_API int fra_focal_check(const fra_focal_spec *spec);
/* k_focal alone, over a host or device raster of any layout into a host or device raster of any layout.  Synchronous.
 * Host buffers are staged as fra_calc stages them (the elements of dst that are not outputs keep the caller's values);
 * the source is read with 16-byte loads and the destination written with vector stores under fra_calc's conditions,
 * judged separately.  left_out (host memory, `channels` words, may be NULL).
 * FRA_E_INVALID, before any GPU work and in this order: a null argument, an invalid spec (fra_focal_check), a bad
 * source or destination dtype or layout (more than 255 bands), an output rectangle that is empty or not inside the
 * source, more than 2^32 pixels per band. */
FRA_API int fra_focal(fra_ctx *ctx, const fra_focal_job *job, uint64_t *left_out /* channels, may be NULL */);
/* The focal operation over what fra_decode_device_window would have written for `roi`, in job->dst_dtype.  roi is the
 * region to decode: the caller has grown the rectangle it wants by the window's radius and clipped it to the raster;
 * `inner` is the output rectangle relative to roi, and the edge mode acts at roi's borders (where the caller's growth
 * was clipped those are the raster's own).  The region never leaves the device; the result goes to `out`, a
 * (job->channels, inner->height, inner->width) raster.  Every refusal and message of the windowed read is this call's as
 * well; items that do not cover roi are refused as by fra_decode_device_compare; the spec and `out` as by fra_focal; an
 * `inner` that is empty or not inside roi is refused.  Afterwards fra_decode_device_timing reports the inner windowed
 * read and fra_focal_timing the map. */
FRA_API int fra_decode_device_focal(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                    const fra_focal_spec *spec, const fra_window *inner, const fra_calc_dst *out,
                                    uint64_t *left_out /* channels, may be NULL */, fra_decoded *infos /* nitems */);
/* HIP-event time (ms) of the calling thread's last k_focal (fra_focal or fra_decode_device_focal) */
FRA_API int fra_focal_timing(float *ms);

/* Zonal statistics: the band statistics of a value raster (channels, h, w) of any fra_dtype, separately for every zone of
 * a zone raster (h, w) of an integer dtype (FRA_U8, FRA_I8, FRA_U16, FRA_I16, FRA_U32 or FRA_I32) with row and column
 * strides of its own: one record per (band, zone).  The fourth classical map-algebra member beside the global
 * (fra_stats, fra_compare), local (fra_calc) and focal (fra_focal) ones.  The reference has no counterpart: its users do
 * this with rasterio + numpy on the host.
 *   Which zone a pixel belongs to.  z = (int64) the zone raster's pixel.  With FRA_ZONAL_IGNORE and z == opts.ignore_zone
 *     the pixel is outside.  Otherwise k = z - opts.zone_lo (exact), and the pixel is outside unless 0 <= k < opts.nzones;
 *     nzones lies in 1 ... 65536.  *outside = the number of pixels of the raster that are outside, one count per call (not
 *     per band).
 *   The record of (band, zone k) is recs[band * nzones + k].  count = the pixels of the zone.  nan, nodata and valid mean
 *     exactly what they mean in fra_stats: every element is taken as f64, nan = the NaN pixels (floats only), nodata = the
 *     pixels with (double)x == opts.nodata, counted only with FRA_ZONAL_NODATA (a NaN nodata matches nothing), valid = the
 *     rest, +-inf are valid numbers; count = valid + nan + nodata.  min, max over the valid pixels, exact doubles, NaN when
 *     valid == 0.
 *   Integer dtypes.  sum (sum_lo uint64, sum_hi int64) and sq (sq_lo, sq_hi) are the exact 128-bit sums of x and x^2 of
 *     fra_stats, in its encoding.  fsum = mean = fm2 = 0.0.  More than 2^32 pixels per band are refused.
 *   f32 / f64.  fsum = the f64 sum of x; mean = fsum / (double)valid, one IEEE division (0 / 0 = NaN for a zone without a
 *     valid pixel); fm2 = the f64 sum of (x - mean) * (x - mean) with that zone's mean of the first pass, read on the device.
 *     Plain IEEE arithmetic: +-inf propagate.  The integer sums are 0.
 *     No summation order is implied, and unlike fra_stats this unit adds fsum and fm2 with f64 atomics (in LDS, then in
 *     device memory): the two of two calls on the same inputs may differ in their last bits.  Everything else in a
 *     record -- the counts, the extremes, mean's relation to fsum, the integer sums -- and `outside` is exact and does not
 *     depend on any order.
 *   A zone without pixels has all counts 0, sums 0, min = max = NaN and, for floats, mean = NaN. */
#define FRA_ZONAL_NODATA 1
#define FRA_ZONAL_IGNORE 2
typedef struct {
  int32_t flags, nzones;
  int64_t zone_lo, ignore_zone;
  double nodata;
} fra_zonal_opts;     /* 32 bytes */
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype */
  int32_t channels, height, width;          /* >= 1 */
  int64_t band_stride, row_stride, col_stride;  /* elements, >= 0 */
  const void *zones; int32_t zones_on_device;   /* element (row 0, col 0) of the zone raster */
  int32_t zone_dtype;                       /* an integer fra_dtype */
  int64_t zone_row_stride, zone_col_stride; /* elements, >= 0 */
  fra_zonal_opts opts;
} fra_zonal_job;
typedef struct {
  uint64_t count, valid, nan, nodata;
  uint64_t sum_lo; int64_t sum_hi; uint64_t sq_lo, sq_hi;
  double   min, max, fsum, mean, fm2;
  uint64_t reserved;  /* 0 */
} fra_zonal_rec;      /* 112 bytes */
/* k_zonal and its small kernels alone, over host or device rasters of any non-negative strides.  Synchronous; recs (host
 * memory) receives channels x nzones records and *outside (host memory) the count.  Host rasters are staged as fra_stats
 * and fra_compare stage theirs (each one allocation spanning every addressed element from element 0); neither raster is
 * written.  Each raster is read with vector loads when its column stride is 1 and its base, row stride (and, for the
 * values, band stride) are multiples of 16 bytes, element by element otherwise, judged separately.  The reference has no
 * counterpart.  FRA_E_INVALID, before any GPU work and in this order: a null argument, a bad value dtype or layout, a zone
 * dtype outside the six, a negative zone stride, nzones outside 1 ... 65536, unknown flag bits, more than 2^32 pixels per
 * band, more than 2^24 records (channels x nzones). */
FRA_API int fra_zonal(fra_ctx *ctx, const fra_zonal_job *job, fra_zonal_rec *recs /* channels x nzones */,
                      uint64_t *outside);
/* The zonal statistics of what fra_decode_device_window would have written for `roi`, in job->dst_dtype.  roi, the items
 * and infos mean what they mean there; job->dst and the job's strides are ignored.  The zone raster (host or device) is
 * addressed relative to the region, exactly as `ref` is in fra_decode_device_compare: the label of pixel (R, C) at
 * (R - roi.row_off)*zone_row_stride + (C - roi.col_off)*zone_col_stride.  The region goes to a per-call device buffer,
 * never leaves the device and is released on every path.  Every refusal and message of the windowed read is this call's
 * as well; items that do not cover the region are refused as by fra_decode_device_compare; the zone raster and the
 * options as by fra_zonal.  The reference has no counterpart.  Afterwards fra_decode_device_timing reports the inner
 * windowed read and fra_zonal_timing the statistics. */
FRA_API int fra_decode_device_zonal(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi, const void *zones,
                                    int32_t zones_on_device, int32_t zone_dtype, int64_t zone_row_stride,
                                    int64_t zone_col_stride, const fra_zonal_opts *opts,
                                    fra_zonal_rec *recs /* channels x nzones */, uint64_t *outside,
                                    fra_decoded *infos /* nitems */);
/* HIP-event time (ms) of the calling thread's last zonal kernels (fra_zonal or fra_decode_device_zonal); the reference
 * has no counterpart */
FRA_API int fra_zonal_timing(float *ms);

/* Warped reads: a raster (channels, H, W) of any fra_dtype, or a region of a set of tile streams, onto an output grid
 * (channels, oh, ow) of its own, 1 <= oh, ow <= 65536, in the input's dtype.  A map takes every output pixel to a source
 * coordinate and the source is sampled there.  The rule (flac_raster/warp.py restates it in numpy: warp_arrays):
 *   All coordinate and value arithmetic is IEEE f64, each operation rounded on its own, no contraction.  Pixel (row r,
 *   col c) covers [c, c + 1) x [r, r + 1); its centre is (c + 0.5, r + 0.5).
 *   Maps.  For output pixel (R, C): u = (double)C + 0.5, v = (double)R + 0.5.
 *     FRA_WARP_AFFINE  six doubles a .. f:  x = (a*u + b*v) + c,  y = (d*u + e*v) + f  -- two products, their sum, then
 *                      the constant, in exactly this order.
 *     FRA_WARP_GRID    step >= 1, gw = ceil(ow / step) + 1, gh = ceil(oh / step) + 1, and two f64 planes gx, gy of shape
 *                      (gh, gw): the source coordinates of the output-grid points (j*step, i*step) -- pixel corners, not
 *                      centres.  cj = min(C / step, gw - 2), ci = min(R / step, gh - 2) (integer division);
 *                      fx = (u - (double)(cj*step)) / (double)step, fy likewise; per plane g
 *                        top = g[ci][cj] + (g[ci][cj+1] - g[ci][cj]) * fx,  bot the same on row ci + 1,
 *                        value = top + (bot - top) * fy.
 *                      (The bilinear coordinate grid of GDAL's approximate transformer: any CRS transform is supplied
 *                      as data, and the kernel and the numpy rule consume the same numbers.)
 *   Inside.  The pixel is inside when x >= 0 && x < W && y >= 0 && y < H, W and H the size of the whole source raster
 *     (not of a decoded region).  A NaN coordinate fails the test.  An outside pixel is written as `fill` and counted
 *     in filled[band].
 *   Sampling an inside pixel.
 *     nearest          in[floor(y)][floor(x)].
 *     bilinear, cubic  px = x - 0.5, i0 = floor(px), t = px - i0, rows likewise.  Taps, weights, the clamping of the tap
 *                      indices to [0, W - 1] / [0, H - 1], the order (vertically first, top to bottom, then left to
 *                      right) and the conversion of the result are exactly those of the resampling rule above, except
 *                      that a NaN result is written as the canonical quiet NaN (0x7ff8000000000000 as the dtype holds
 *                      it), so that a float output is fixed to the last bit (the nearest copies its pixel's bits).
 *     With FRA_WARP_NODATA the validity of a value and the renormalisation are exactly those of the nodata-aware rule's
 *     "bilinear, cubic" paragraph and its "nearest" line: all taps valid gives the unmasked formula; otherwise the
 *     masked bilinear of the same centre; no valid tap, or Wt <= 0, gives `fill` and the pixel is counted.  The nearest
 *     picks its pixel, invalid or not, and counts it when it is invalid.  Without the flag NaN and +-inf propagate.
 *     `fill` is a double the dtype admits by the nodata rule (an integer in range; for floats NaN, or finite and exact);
 *     so is `nodata` under FRA_WARP_NODATA.  FRA_RESAMPLE_AVERAGE is refused: a warp that shrinks takes point samples
 *     (read an overview first, then warp that).
 *   Consequences.  Under the identity map (1, 0, 0, 0, 1, 0) the nearest returns the input bit for bit, and the bilinear
 *     and the cubic return every finite value (t = 0: the other taps weigh 0.0, so -0.0 comes back as +0.0, and a tap
 *     of +-inf or NaN next to a pixel makes it NaN).  An integer translation is, likewise, a shifted copy with fill.
 *     For an axis-aligned map whose scales are powers of two and whose offsets are 0 every coordinate is exact, and the
 *     result equals fra_resample / fra_resample_masked (nearest, bilinear, cubic) of that size bit for bit (for the
 *     masked ones when `fill` is the nodata value; a NaN result has the sign the hardware gives it there, none here).
 * k_warp: one 256-thread workgroup per 16 x 64 output tile of a band; every thread computes the source coordinates of
 * its pixels and reads its taps from global memory ("gathered").  A second path that staged the tile's footprint in LDS
 * ("staged") was measured slower and is not built; fra_warp_paths still reports both counts. */
#define FRA_WARP_AFFINE 0
#define FRA_WARP_GRID 1
#define FRA_WARP_NODATA 1
typedef struct {
  int32_t kind;                             /* FRA_WARP_AFFINE, FRA_WARP_GRID */
  int32_t step, gh, gw;                     /* GRID: the step and the planes' shape */
  double affine[6];                         /* AFFINE: a .. f, finite */
  const double *gx, *gy;                    /* GRID: host memory, gh * gw doubles each, row-major */
} fra_warp_map;                             /* 80 bytes */
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype, of src and dst */
  int32_t channels, height, width;          /* >= 1; channels <= 255 */
  int64_t src_band_stride, src_row_stride, src_col_stride;  /* elements, >= 0 */
  int32_t out_height, out_width;            /* 1 .. FRA_RESAMPLE_MAX_OUT */
  int32_t resampling;                       /* FRA_RESAMPLE_NEAREST, _BILINEAR, _CUBIC */
  int32_t flags;                            /* FRA_WARP_NODATA */
  void *dst; int32_t dst_on_device;         /* (channels, out_height, out_width) through the strides below */
  int64_t dst_band_stride, dst_row_stride, dst_col_stride;
  double nodata, fill;
  fra_warp_map map;
} fra_warp_job;                             /* 208 bytes */
/* k_warp alone, over a host or device raster of any dtype and layout.  Synchronous.  Host buffers are staged as
 * fra_resample stages them (the elements of dst that are not outputs keep the caller's values).  filled (host memory,
 * `channels` words, may be NULL) receives per band the number of output pixels written as the fill (and the invalid
 * pixels the nearest picked).
 * FRA_E_INVALID, before any GPU work: a null argument, a bad dtype or layout (more than 255 bands), an output size
 * outside 1 .. 65536, an unknown or AVERAGE resampling, unknown flags, an unknown map kind, step < 1 or gh / gw that do
 * not match step, a null grid, a non-finite affine coefficient, a nodata or fill the dtype does not admit. */
FRA_API int fra_warp(fra_ctx *ctx, const fra_warp_job *job, uint64_t *filled /* channels, may be NULL */);
/* The warp of what fra_decode_device would have written for the whole raster_h x raster_w raster the items tile, in
 * dst_dtype.  The host computes the source window the map touches -- for an affine map from the four corner pixel
 * centres of the output, for a grid map from the grid nodes alone (a bilinear patch has its extremes at its corners;
 * non-finite nodes are left out) --, grows it by 3 pixels per side and clips it to the raster
 * (fra_warp_source_window).  That window is decoded by the windowed read into a per-call device buffer (its refusals and
 * messages are this call's; the items must cover the window), then k_warp runs with the window's origin: taps are
 * clamped against the whole raster and indexed relative to the window.  The job's dst and strides address the out_h x
 * out_w output.  A footprint wholly outside the raster (by more than a pixel) decodes nothing (infos are zeroed), writes the fill everywhere
 * and returns FRA_OK with filled = out_h * out_w per band.  FRA_E_INVALID before any GPU work for everything fra_warp
 * refuses so, and for a raster size below 1.  Afterwards fra_decode_device_timing reports the inner windowed read and
 * fra_warp_timing the warp. */
FRA_API int fra_decode_device_warped(fra_ctx *ctx, const fra_decode_job *job, int32_t raster_h, int32_t raster_w,
                                     const fra_warp_map *map, int32_t out_h, int32_t out_w, int32_t resampling,
                                     int32_t flags, double nodata, double fill, fra_decoded *infos /* nitems */,
                                     uint64_t *filled /* channels, may be NULL */);
/* The source window fra_decode_device_warped decodes for a checked map: *window; returns 0 when the footprint lies wholly
 * outside the raster (nothing is decoded), 1 otherwise, FRA_E_INVALID for what fra_warp refuses in a map or a size.
 * Pure host code: no context, no GPU. */
FRA_API int fra_warp_source_window(const fra_warp_map *map, int32_t raster_h, int32_t raster_w, int32_t out_h,
                                   int32_t out_w, fra_window *window);
/* HIP-event time (ms) of the calling thread's last k_warp (fra_warp or fra_decode_device_warped) */
FRA_API int fra_warp_timing(float *ms);
/* The workgroups of the calling thread's last k_warp that staged their taps in LDS (counts[0]: always 0, no such path is
 * built) and that gathered them from global memory (counts[1]: all of them) */
FRA_API int fra_warp_paths(uint64_t counts[2]);

/* Rasterizing polygons: vector features burned into an integer raster -- zones and masks for the units above -- by a rule
 * that flac_raster/rasterize.py restates in numpy (rasterize_arrays).  All arithmetic is IEEE f64, every operation
 * rounded on its own, nothing contracted.
 *   Input: nfeatures features in order.  Feature f is the rings feature_ring_start[f] .. feature_ring_start[f + 1] - 1,
 *     ring r the vertices ring_start[r] .. ring_start[r + 1] - 1 of xy (x, y interleaved), at least 3 of them, in PIXEL
 *     coordinates of the raster the output window belongs to (x along columns, y along rows).  Exterior rings, holes
 *     and the parts of a multipolygon are not told apart.  values[f] is the feature's burn value.  All of these arrays
 *     are host memory.
 *   Output: the window (row_off, col_off, height, width).  Pixel (r, c) has the centre
 *     xc = (double)(col_off + c) + 0.5, yc = (double)(row_off + r) + 0.5.
 *   Edges: a ring is closed implicitly (last -> first; a repeated closing vertex gives an edge of no length, dropped
 *     next).  An edge with y0 == y1 is dropped.  Every other edge is oriented so that y0 < y1, its endpoints swapped if
 *     need be before any arithmetic: two features that share an edge compute the same numbers for it.
 *   Crossing: an edge crosses the scanline of yc when y0 <= yc && yc < y1.  Then t = (yc - y0) / (y1 - y0) and
 *     xi = x0 + t * (x1 - x0); the edge counts for the pixel when xi > xc.
 *   Coverage: a feature covers the pixel when an odd number of its edges count, over all its rings (even-odd).
 *   Burn: the pixel's value is the burn value of the covering feature with the highest index (painter's order, as GDAL
 *     burns); `fill` without one.  *burned: the pixels of the window covered by at least one feature.
 *   Output dtype: FRA_U8, FRA_I8, FRA_U16, FRA_I16, FRA_U32 or FRA_I32 (the zone dtypes of fra_zonal).
 * So the square [2.5, 10.5] x [2.5, 8.5] covers columns 2..9 and rows 2..7 (half-open on both axes), two features
 * that share an edge never both cover a pixel nor both miss one between them, and the result does not depend on a
 * ring's orientation, on its first vertex or on any binning.
 *   FRA_E_INVALID before any GPU work, in this order: a null argument (ctx, job, dst; a geometry array that its count
 *   makes needed); a dtype outside the six; height or width outside 1 .. 65536; a negative stride; negative counts,
 *   feature_ring_start not ascending from 0 to nrings, ring_start not ascending from 0 or past nverts; a ring of fewer
 *   than 3 vertices; a coordinate that is not finite or above 2^52 in magnitude; a burn value, then a fill, the dtype
 *   does not hold; more than 2^24 features; more than 2^28 vertices.  nfeatures == 0 is valid: the fill everywhere,
 *   *burned = 0.  FRA_E_NOMEM when the band lists below would pass 2^31 - 1 entries.
 * The host builds the edge table and one list of edges per band of 16 output rows (an edge is in the list of every band
 * one of whose row centres its [y0, y1) contains; feature order, and edge order within a feature, are kept).
 * k_rasterize: one 256-thread workgroup per 16 x 64 output tile walks its band's list in chunks, computes xi once per
 * (edge, row) into LDS and lets every thread toggle the parity of its 4 pixels (fra_rasterize.hip). */
typedef struct {
  const double *xy;                     /* nverts x (x, y) */
  int64_t nverts;
  const int64_t *ring_start;            /* nrings + 1 */
  int64_t nrings;
  const int64_t *feature_ring_start;    /* nfeatures + 1 */
  int32_t nfeatures;
  const int64_t *values;                /* nfeatures */
  int32_t dtype;                        /* of the output */
  int64_t row_off, col_off;
  int32_t height, width;
  int64_t fill;
  void *dst;
  int32_t dst_on_device;
  int64_t row_stride, col_stride;       /* in elements, non-negative */
} fra_rasterize_job;                    /* 128 bytes */
/* Synchronous.  A host dst is staged whole, from its element 0 to the last one addressed, and copied back whole (as
 * fra_warp stages it): the elements between the outputs keep the caller's values.  Every device allocation is per call
 * and released on every path. */
FRA_API int fra_rasterize(fra_ctx *ctx, const fra_rasterize_job *job, uint64_t *burned /* may be NULL */);
/* HIP-event time (ms) of the calling thread's last k_rasterize and its fold */
FRA_API int fra_rasterize_timing(float *ms);

/* Proximity: for every pixel of a region the exact Euclidean distance to the nearest target pixel, and the source
 * value at that target (nearest-target allocation) -- buffers around burned features, distance to water, a mask grown by
 * a radius.  flac_raster/proximity.py restates the rule in numpy (proximity_direct: all pairs; proximity_arrays: the
 * separable form).  Squared pixel distances are integers, so everything up to the one f64 square root is exact.
 *   Region: a (channels, h, w) raster of any fra_dtype, 1 <= h, w <= 32768 (every squared distance is below 2^31).  Each
 *     band is handled on its own.  Targets outside the region do not exist.
 *   Targets: with nvalues == 0 a pixel is a target when its value is non-zero and not NaN (-0.0 is zero); with
 *     1 <= nvalues <= 16 when (double)v == values[i] for some i (so NaN never is).
 *   Squared distance of pixel (r, c): d2 = min over the band's targets (r', c') of (r - r')^2 + (c - c')^2, in integers.
 *     A band without a target has no d2.
 *   Nearest target: among the targets at that minimum the one with the smallest column, among those the one with the
 *     smallest row.
 *   Distance: d = sqrt((double)d2) * scale in f64, each operation rounded on its own; scale is finite and > 0 (1: pixel
 *     units; the pixel size: map units).
 *   Reach: a pixel is within reach when it has a d2 and either has_max_dist is 0 or d <= max_dist in f64.  (d is
 *     monotone in d2, so the host turns this into the greatest d2 within reach, exactly.)
 *   dist output (optional, any fra_dtype; dist.dst == NULL: not wanted): a pixel within reach gets d, or `fixed` when
 *     has_fixed is set -- a target included: a buffer contains its core; every other pixel gets `fill`.  All three are
 *     converted as the band math converts a result (Output, above).
 *   alloc output (optional, the source's dtype; alloc.dst == NULL: not wanted; alloc.dtype is ignored): a pixel within
 *     reach gets the source value at its nearest target, bits copied; every other pixel gets alloc_fill, converted as
 *     above.
 *   Output window: only the pixels (out_row_off, out_col_off, out_height, out_width) of the region are written, at
 *     dst[band, r - out_row_off, c - out_col_off] through the output's strides; targets anywhere in the region count.
 *     So a window of a large raster is exact under a max_dist: the caller passes the window grown by
 *     ceil(max_dist / scale) pixels, clipped to the raster, as the region.
 *   counts[0]: the targets in the region; counts[1]: the output-window pixels within reach; counts[2]: the
 *     output-window pixels that got the fill; each summed over the bands.
 * Two phases.  Columns (k_prox_mask, k_prox_carry, k_prox_cols): per pixel of the output window's rows the vertical
 * distance g to the nearest target of its own column and whether it lies above or below (above wins a tie; g beyond the
 * reach is "none"), 16 bits per pixel, from one 64-bit target mask per 64 rows of a column.  Rows (k_prox_rows): per
 * output row d2[c] = min over c' of g[c']^2 + (c - c')^2, the leftmost c' winning a tie; that argmin does not decrease
 * with c, so the row is solved by divide and conquer in LDS, every level in parallel (fra_proximity.hip). */
typedef struct {
  int32_t nvalues;                          /* 0 .. 16 */
  int32_t has_max_dist, has_fixed;
  int32_t out_row_off, out_col_off, out_height, out_width;  /* the output window, inside the region */
  int32_t reserved;
  double values[16];
  double scale, max_dist, fixed, fill, alloc_fill;
  fra_calc_dst dist;                        /* (channels, out_height, out_width) of dist.dtype; dst NULL: none */
  fra_calc_dst alloc;                       /* (channels, out_height, out_width) of the source's dtype; dst NULL: none */
} fra_proximity_opts;                       /* 280 bytes */
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype of the source */
  int32_t channels, height, width;          /* channels 1 .. 255; height, width 1 .. 32768 */
  int64_t band_stride, row_stride, col_stride;  /* elements, >= 0 */
  fra_proximity_opts opts;
} fra_proximity_job;
/* Over a host or device raster of any layout into host or device rasters of any layout.  Synchronous.  Host buffers are
 * staged as fra_calc stages them (the elements of an output that are not outputs keep the caller's values).  The
 * scratch (the masks, the carries and one band's 16-bit intermediate at a time) is per call and released on every path.
 * counts (host memory, 3 words) may be NULL.
 * FRA_E_INVALID, before any GPU work and in this order: a null argument (ctx, job, src); a bad source dtype or layout
 * (more than 255 bands), a bad dtype or a negative stride of an output that is given; height or width outside
 * 1 .. 32768; nvalues outside 0 .. 16 or a value that is not finite; a scale that is not finite and positive; with
 * has_max_dist a max_dist that is NaN or negative (+inf is no limit); an output window that is empty or leaves the
 * region; neither output given. */
FRA_API int fra_proximity(fra_ctx *ctx, const fra_proximity_job *job, uint64_t *counts /* 3, may be NULL */);
/* The same over what fra_decode_device_window would have written for `roi`, in job->dst_dtype: roi is the region
 * (opts' output window is relative to it), job->dst and the job's strides are ignored, and the decoded region never
 * leaves the device.  Every refusal and message of the windowed read is this call's as well; items that do not cover
 * roi are refused as by fra_decode_device_compare; the options and outputs as by fra_proximity.  Afterwards
 * fra_decode_device_timing reports the inner windowed read and fra_proximity_timing the transform. */
FRA_API int fra_decode_device_proximity(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                        const fra_proximity_opts *opts, fra_decoded *infos /* nitems */,
                                        uint64_t *counts /* 3, may be NULL */);
/* HIP-event times (ms) of the calling thread's last proximity call: ms[0] the column phase, ms[1] the row phase, each
 * summed over the bands */
FRA_API int fra_proximity_timing(float ms[2]);

/* Regions: the connected components of a raster's foreground, their areas and boxes, and a sieve that removes the small
 * ones -- "how many water bodies, how big, where", "drop the specks below 20 pixels", "a zone per field".
 * flac_raster/regions.py restates the rule in numpy (regions_direct: a flood fill; regions_arrays: run-based union-find).
 * Everything is integer work, so the GPU result equals the rule byte for byte, and is the same from run to run.
 *   Region: a (channels, h, w) raster of any fra_dtype, 1 <= h, w <= 32768 (every pixel index and every area is below
 *     2^31).  Each band is handled on its own.  Pixels outside the region do not exist: a component is cut at the
 *     region's edge, so a window of a raster labels the window.  There is no output window.
 *   Foreground: the targets of the proximity rule (above): with nvalues == 0 a pixel whose value is non-zero and not NaN,
 *     with 1 <= nvalues <= 16 one with (double)v == values[i] for some i.  invert (0 / 1) swaps foreground and
 *     background after that test; a NaN stays background.  values = {nodata}, invert = 1 is "everything but nodata".
 *   Links: connectivity is 4 (W, E, N, S) or 8 (the diagonals too).  Two neighbouring foreground pixels are linked when
 *     by_value == 0; with by_value == 1 only if their values are also equal under == in the source dtype (-0.0 == 0.0).
 *     A component is a class of the transitive closure of the links.
 *   First pixel, area, box: a component's first pixel is its pixel with the smallest r * w + c; its area is its pixel
 *     count; its box is the minimum and maximum of its rows and of its columns.
 *   Sieve: min_size >= 1.  A component is kept when area >= min_size and removed otherwise (1 keeps everything).
 *   Numbering: the kept components of a band are numbered 1 .. N in the order of their first pixels.  Background pixels
 *     and the pixels of removed components have label 0.
 *   Outputs, each optional (dst == NULL: not wanted), at least one of the three rasters or the table:
 *     labels (an integer fra_dtype): the number of the pixel's kept component, 0 elsewhere;
 *     area (any fra_dtype): the area of the pixel's kept component, 0 elsewhere, converted as the band math converts a
 *       result (Output, above);
 *     sieved (the source's dtype; sieved.dtype is ignored): the source bits, except that the pixels of removed components
 *       get sieve_fill, converted as the proximity rule converts its fills;
 *     table: table_cap records per band, in host memory or (table_on_device) device memory; record i - 1 of a band
 *       describes its kept component i.  The value of a component is the source at `first`.
 *   counts[4 * band + k]: k = 0 the foreground pixels, 1 the components before the sieve, 2 the kept components N, 3 the
 *     pixels of kept components.
 *   Refused after the counts are known, FRA_E_SPACE: N of some band exceeds the maximum of the labels dtype, or
 *     table_cap.  The message names the band, N and the limit; counts is complete and no element of any output has been
 *     written.
 * Four phases (fra_regions.hip): k_reg_links turns the source into one byte per pixel (foreground and the links towards
 * W, N, NW, NE) -- every later kernel reads only these; k_reg_tile labels tiles of 64 x 64 pixels by union-find in LDS
 * and writes every pixel's parent as a pixel index; k_reg_seam unites across the tile borders on that array with
 * atomicMin; then every pixel finds its root (the component's first pixel), the roots are numbered in raster order by
 * a prefix sum, areas and boxes are accumulated with integer atomics (merged per thread run and per workgroup first),
 * the kept components are numbered by a second prefix sum and a last pass writes the outputs.  No kernel waits for
 * another workgroup. */
typedef struct {
  uint32_t first;                           /* r * w + c of the component's first pixel */
  uint32_t area;
  int32_t rmin, cmin, rmax, cmax;
} fra_region_rec;                           /* 24 bytes */
typedef struct {
  int32_t nvalues;                          /* 0 .. 16 */
  int32_t invert, by_value;                 /* 0 / 1 (non-zero: 1) */
  int32_t connectivity;                     /* 4 or 8 */
  int32_t min_size;                         /* >= 1 */
  int32_t table_cap;                        /* records per band that `table` holds, >= 0 */
  int32_t table_on_device, reserved;
  double values[16];
  double sieve_fill;
  fra_region_rec *table;                    /* channels x table_cap records; NULL: none */
  fra_calc_dst labels;                      /* (channels, h, w) of labels.dtype, an integer one; dst NULL: none */
  fra_calc_dst area;                        /* (channels, h, w) of area.dtype; dst NULL: none */
  fra_calc_dst sieved;                      /* (channels, h, w) of the source's dtype; dst NULL: none */
} fra_regions_opts;                         /* 296 bytes */
typedef struct {
  const void *src; int32_t src_on_device;   /* element (band 0, row 0, col 0); host memory is copied to the device */
  int32_t dtype;                            /* fra_dtype of the source */
  int32_t channels, height, width;          /* channels 1 .. 255; height, width 1 .. 32768 */
  int64_t band_stride, row_stride, col_stride;  /* elements, >= 0 */
  fra_regions_opts opts;
} fra_regions_job;
/* Over a host or device raster of any layout into host or device rasters of any layout.  Synchronous.  Host buffers are
 * staged as fra_proximity stages them (the elements of an output that are not outputs keep the caller's values; a host
 * table is written record by record up to N per band).  The scratch -- one band at a time: a link byte and a 4-byte
 * parent per pixel, and 28 bytes per component before the sieve -- is per call and released on every path.  With more
 * than one band and a possible FRA_E_SPACE (a table, or a labels dtype narrower than 31 bits) every band is counted
 * before any is written, so the bands are labelled twice.  counts (host memory, 4 words per band) may be NULL.
 * FRA_E_INVALID, before any GPU work and in this order: a null argument (ctx, job, src); a bad source dtype or layout
 * (more than 255 bands); a labels dtype that is not an integer one; a bad dtype or a negative stride of an output that
 * is given; height or width outside 1 .. 32768; nvalues outside 0 .. 16 or a value that is not finite; a connectivity
 * other than 4 or 8; min_size < 1; table_cap < 0; no output given. */
FRA_API int fra_regions(fra_ctx *ctx, const fra_regions_job *job, uint64_t *counts /* 4 per band, may be NULL */);
/* The same over what fra_decode_device_window would have written for `roi`, in job->dst_dtype: roi is the region,
 * job->dst and the job's strides are ignored, and the decoded region never leaves the device.  Every refusal and message
 * of the windowed read is this call's as well; items that do not cover roi are refused as by fra_decode_device_compare;
 * the options and outputs as by fra_regions.  Afterwards fra_decode_device_timing reports the inner windowed read and
 * fra_regions_timing the labelling. */
FRA_API int fra_decode_device_regions(fra_ctx *ctx, const fra_decode_job *job, const fra_window *roi,
                                      const fra_regions_opts *opts, fra_decoded *infos /* nitems */,
                                      uint64_t *counts /* 4 per band, may be NULL */);
/* HIP-event times (ms) of the calling thread's last regions call, each summed over the bands and over both rounds when
 * the bands are labelled twice: ms[0] the links, ms[1] the tile labelling, ms[2] the seams, ms[3] the kernels after them
 * (flatten, count, number, write; the waits for the two counts the host reads back lie between its three stretches of
 * kernels and are not in it). */
FRA_API int fra_regions_timing(float ms[4]);

/* Verify (libFLAC's verify mode for a plan): after an execute (or fra_plan_encode_host / _progress / _ring) has
 * completed, decode the plan's own frames on its GPU through its frame offsets -- k_dec_parse with every CRC-16,
 * k_dec_restore -- and compare every decoded sample with the plan's current raster (the caller's device raster, or the
 * plan's own copy of a host raster) normalised anew by the plain f64 operation sequence with the min / max of the last
 * execute, read on the device (k_dec_verify; norm == 0: the raw int16 / int32).  No second raster is allocated and
 * nothing is written back; scratch is that of fra_decode_device, allocated per call and freed on every path.
 *   Returns FRA_OK whether or not samples differ: a mismatch is a result.  reports[w] describes window w and
 * *bad_windows counts the windows with mismatches > 0.  first_sample / first_channel name the first mismatch in the
 * stream's sample order (pixel, then channel); first_sample is the window-relative pixel index (row = first_sample /
 * width, column = first_sample % width of the window), also for a ranged plan (fra_plan_create_ranged), which is
 * verified over its own frames only.  A raster the caller has overwritten since the execute simply reports mismatches.
 *   FRA_E_INVALID for a null argument (before the plan is looked at) and, with the decoder's message ("lost sync /
 * corrupt frame at byte N", N relative to the window's first frame), for a frame that does not parse or whose CRC-16
 * fails; FRA_E_STATE before the first execute.  Synchronous.  Afterwards fra_decode_device_timing reports k_dec_parse,
 * k_dec_restore and, in slot 2, k_dec_verify. */
typedef struct {
  uint64_t mismatches;    /* samples (counted per channel) that differ from the normalised input */
  int64_t  first_sample;  /* window-relative pixel index of the first mismatch in (pixel, channel) order; -1: none */
  int32_t  first_channel;
  int32_t  expected, got; /* normalised input sample / decoded sample there (0 when none) */
  int32_t  nframes;       /* frames decoded, each with a valid CRC-16 */
} fra_verify_report;      /* 32 bytes */
FRA_API int fra_plan_verify(fra_plan *plan, fra_verify_report *reports /* nwindows */, int32_t *bad_windows);

/* Synthetic rasters, generated on the device with integer-exact hashes so a
 * host numpy mirror reproduces any window bit for bit.  kind: 3 = C3 DEM int16, 4 = C4 S2-like
 * uint16 (4 bands), 5 = C5 reflectance float32.  dev_out: device buffer (bands, height, width). */
FRA_API int fra_synth_raster(fra_ctx *ctx, int32_t kind, uint64_t seed, int32_t bands, int32_t height, int32_t width,
                     void *dev_out);

/* GeoTIFF chunk decoder (host, multi-threaded; raster I/O ahead of the path, SURVEY.md 8(f) f3,
 * replacing rasterio's window reads at cli.py:559 / converter.py:73-79 / spatial_encoder.py:205-206).
 * The caller parses the IFD and lists the strips/tiles overlapping the window; each is decompressed
 * (none, LZW, deflate), un-predicted (1, 2 horizontal, 3 floating point) and its overlap with the
 * window written band-planar into dst (element (b, r, c) of the window at
 * b*dst_band_stride + r*dst_row_stride + c, native byte order).  threads <= 0: hardware concurrency. */
typedef struct {
  uint64_t offset, bytes;   /* compressed chunk within the file buffer */
  int32_t row0, col0;       /* image position of the chunk's first pixel */
  int32_t rows, cols;       /* chunk extent as stored (full tile, or strip rows x image width) */
  int32_t plane;            /* band of a planar (PlanarConfiguration 2) chunk; ignored when chunky */
  int32_t pad;
} fra_tiff_chunk;
typedef struct {
  int32_t compression;        /* 1, 5 (LZW), 8 or 32946 (deflate) */
  int32_t predictor;          /* 1, 2, 3 */
  int32_t bytes_per_sample;   /* 1, 2, 4, 8 */
  int32_t samples_per_pixel;  /* per chunk: SamplesPerPixel when chunky, 1 when planar */
  int32_t is_float;           /* SampleFormat 3 */
  int32_t big_endian;         /* MM file */
  int32_t bands;              /* bands of the destination */
  int32_t win_row, win_col, win_h, win_w;  /* destination window in image pixels */
  int32_t pad;
  int64_t dst_band_stride, dst_row_stride; /* elements */
} fra_tiff_layout;
FRA_API int fra_tiff_decode(const uint8_t *file, uint64_t file_len, const fra_tiff_layout *layout,
                            const fra_tiff_chunk *chunks, int32_t nchunks, void *dst, int32_t threads);

/* GeoTIFF chunk encoder (host, multi-threaded; the write side of the raster I/O, replacing rasterio's
 * tile GeoTIFF writes at cli.py:577-591 / converter.py flac_to_tiff): nchunks raw chunks of chunk_bytes
 * each, contiguous in src (already in file layout, predictor applied by the caller), are compressed with
 * compression 5 (TIFF LZW, MSB-first, early change -- what fra_tiff_decode and libtiff read) or 8 (zlib
 * deflate at `level`); chunk i goes to dst + i * dst_stride (dst_stride >= fra_tiff_compress_bound) and its
 * size to sizes[i]. */
FRA_API uint64_t fra_tiff_compress_bound(int32_t compression, uint64_t chunk_bytes);
FRA_API int fra_tiff_compress(int32_t compression, int32_t level, const uint8_t *src, uint64_t chunk_bytes,
                              int32_t nchunks, uint8_t *dst, uint64_t dst_stride, uint64_t *sizes, int32_t threads);

/* device memory helpers for hosts without a GPU array library */
FRA_API int fra_device_alloc(fra_ctx *ctx, uint64_t bytes, void **dev_ptr);
FRA_API int fra_device_free(fra_ctx *ctx, void *dev_ptr);
FRA_API int fra_memcpy_d2h(fra_ctx *ctx, void *dst, const void *src, uint64_t bytes);
FRA_API int fra_memcpy_h2d(fra_ctx *ctx, void *dst, const void *src, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* FLAC_RASTER_AMD_H */
