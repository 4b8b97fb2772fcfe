// pft_depth.hip -- the depth entrance of the input filters (include/pft_filters.h): a registered
// depth image and colour image cross the bus (5 bytes per pixel at qhd instead of the 32-byte record) and the organised
// cloud the reference subscribes to (/kinect2/qhd/points, auto_tracking.cpp:775) is formed here, in the filter handle's
// own input buffer.  The pipeline of pft_filters.hip then runs over it on the same stream, unchanged.
//
// k_depth_deproject is a pure streaming kernel: one lane per pixel, 2 - 4 bytes of depth and 0 - 4 bytes of colour read,
// two 16-byte stores written, so a wave writes one contiguous 2 KB.  The reads are the plainest correct form: an aligned
// sample is one load, a sample whose row stride breaks its alignment is read byte by byte.
#include <math.h>
#include <string.h>

#include <string>

#include "pft_devbuf.h"
#include "pft_internal.h"
#include "../../include/pft_filters.h"

#define DP_THREADS 256
#define DP_PAD 16  // bytes behind the device copies of the images

struct DpParams {
  uint32_t n, W;
  float ifx, ify, cx, cy, divisor;
  int depth_format, color_format;
  uint32_t depth_stride, color_stride;
  int depth_aligned, color_aligned;  // every sample / 4-byte pixel lies at a multiple of its size
};

__device__ __forceinline__ uint32_t dp_load_u16(const uint8_t* p, int aligned) {
  if (aligned) return *reinterpret_cast<const uint16_t*>(p);
  return (uint32_t)p[0] | (uint32_t)p[1] << 8;
}
__device__ __forceinline__ uint32_t dp_load_u32(const uint8_t* p, int aligned) {
  if (aligned) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__global__ __launch_bounds__(DP_THREADS) void k_depth_deproject(DpParams p, const uint8_t* __restrict__ depth,
                                                                const uint8_t* __restrict__ color,
                                                                pft_point_xyzrgba* __restrict__ out) {
  const uint32_t i = blockIdx.x * DP_THREADS + threadIdx.x;
  if (i >= p.n) return;
  const uint32_t r = i / p.W, c = i - r * p.W;
  bool valid;
  float z;
  if (p.depth_format == PFT_DEPTH_U16) {
    const uint32_t d = dp_load_u16(depth + (size_t)r * p.depth_stride + (size_t)c * 2u, p.depth_aligned);
    valid = d != 0u;
    z = (float)d / p.divisor;
  } else {
    z = __uint_as_float(dp_load_u32(depth + (size_t)r * p.depth_stride + (size_t)c * 4u, p.depth_aligned));
    valid = __builtin_isfinite(z) && z > 0.0f;
  }
  float4 a = make_float4(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), 1.0f);
  uint32_t rgba = 0u;
  if (valid) {
    const float lx = ((float)c - p.cx) * p.ifx;
    const float ly = ((float)r - p.cy) * p.ify;
    a.x = lx * z;
    a.y = ly * z;
    a.z = z;
    uint32_t c0 = 0u, c1 = 0u, c2 = 0u;  // the first three bytes of the pixel
    if (p.color_format == PFT_COLOR_BGR8 || p.color_format == PFT_COLOR_RGB8) {
      const uint8_t* q = color + (size_t)r * p.color_stride + (size_t)c * 3u;
      c0 = q[0];
      c1 = q[1];
      c2 = q[2];
    } else if (p.color_format != PFT_COLOR_NONE) {
      const uint32_t w = dp_load_u32(color + (size_t)r * p.color_stride + (size_t)c * 4u, p.color_aligned);
      c0 = w & 255u;
      c1 = (w >> 8) & 255u;
      c2 = (w >> 16) & 255u;
    }
    const bool bgr = p.color_format == PFT_COLOR_BGR8 || p.color_format == PFT_COLOR_BGRA8;
    rgba = 0xff000000u | (bgr ? c2 : c0) << 16 | c1 << 8 | (bgr ? c0 : c2);
  }
  float4* o = reinterpret_cast<float4*>(out + i);
  o[0] = a;
  o[1] = make_float4(__uint_as_float(rgba), 0.0f, 0.0f, 0.0f);
}

// ---------------------------------------------------------------------------------------------------
// host side
struct DpSlot {
  void* depth = nullptr;
  void* color = nullptr;
  size_t depth_bytes = 0, color_bytes = 0;
  hipEvent_t ev = nullptr;  // behind the last upload from this slot
  bool recorded = false;
};

struct PftDepthState {
  uint8_t* d_depth = nullptr;
  uint8_t* d_color = nullptr;
  size_t cap_depth = 0, cap_color = 0;
  hipEvent_t ev_up = nullptr;  // behind the upload of caller memory
  DpSlot slot[PFT_DEPTH_SLOTS];
};

void pftd_destroy(PftDepthState* s) {
  if (!s) return;
  pft_dfree(s->d_depth);
  pft_dfree(s->d_color);
  if (s->ev_up) hipEventDestroy(s->ev_up);
  for (DpSlot& q : s->slot) {
    if (q.depth) hipHostFree(q.depth);
    if (q.color) hipHostFree(q.color);
    if (q.ev) hipEventDestroy(q.ev);
  }
  delete s;
}

struct DpLayout {
  uint32_t depth_stride, color_stride;  // resolved (0 = packed)
  size_t depth_bytes, color_bytes;      // through the last pixel of the last row
  size_t n;
};

static uint32_t dp_depth_bpp(int fmt) { return fmt == PFT_DEPTH_U16 ? 2u : 4u; }
static uint32_t dp_color_bpp(int fmt) { return fmt == PFT_COLOR_NONE ? 0u : (fmt <= PFT_COLOR_RGB8 ? 3u : 4u); }

static int dp_invalid(std::string* err, const char* field, const char* why) {
  *err = std::string("pft_depth_frame: ") + field + " " + why;
  return PFT_ERR_INVALID_ARG;
}

// the description alone (no pointers): every error of include/pft_filters.h but the two pointer ones
static int dp_validate(const pft_depth_frame* d, std::string* err, DpLayout* L) {
  if (!d) return dp_invalid(err, "description", "is null");
  if (d->abi_version != PFT_ABI_VERSION) return dp_invalid(err, "abi_version", "is not PFT_ABI_VERSION");
  if (d->width < 1) return dp_invalid(err, "width", "must be >= 1");
  if (d->height < 1) return dp_invalid(err, "height", "must be >= 1");
  if (!(isfinite(d->fx) && d->fx > 0.0f)) return dp_invalid(err, "fx", "must be finite and > 0");
  if (!(isfinite(d->fy) && d->fy > 0.0f)) return dp_invalid(err, "fy", "must be finite and > 0");
  if (!isfinite(d->cx)) return dp_invalid(err, "cx", "must be finite");
  if (!isfinite(d->cy)) return dp_invalid(err, "cy", "must be finite");
  if (d->depth_format != PFT_DEPTH_U16 && d->depth_format != PFT_DEPTH_F32)
    return dp_invalid(err, "depth_format", "is not PFT_DEPTH_U16 or PFT_DEPTH_F32");
  if (d->depth_format == PFT_DEPTH_U16 && !(isfinite(d->depth_divisor) && d->depth_divisor > 0.0f))
    return dp_invalid(err, "depth_divisor", "must be finite and > 0");
  if (d->color_format < PFT_COLOR_NONE || d->color_format > PFT_COLOR_RGBA8)
    return dp_invalid(err, "color_format", "is not one of PFT_COLOR_*");
  if (d->width > PFT_DEPTH_MAX_AXIS || d->height > PFT_DEPTH_MAX_AXIS) {
    *err = "pft_depth_frame: width and height are limited to PFT_DEPTH_MAX_AXIS (16384) each";
    return PFT_ERR_CAPACITY;
  }
  const size_t W = (size_t)d->width, H = (size_t)d->height;
  if (W * H > 0x7fffffffu) {
    *err = "pft_depth_frame: width x height is above what the pipeline takes";
    return PFT_ERR_CAPACITY;
  }
  const size_t drow = W * dp_depth_bpp(d->depth_format), crow = W * dp_color_bpp(d->color_format);
  if (d->depth_stride && d->depth_stride < drow) return dp_invalid(err, "depth_stride", "is shorter than a row of pixels");
  if (d->color_format != PFT_COLOR_NONE && d->color_stride && d->color_stride < crow)
    return dp_invalid(err, "color_stride", "is shorter than a row of pixels");
  L->depth_stride = d->depth_stride ? d->depth_stride : (uint32_t)drow;
  L->color_stride = d->color_format == PFT_COLOR_NONE ? 0u : (d->color_stride ? d->color_stride : (uint32_t)crow);
  L->depth_bytes = (H - 1) * L->depth_stride + drow;
  L->color_bytes = crow ? (H - 1) * L->color_stride + crow : 0;
  L->n = W * H;
  return PFT_OK;
}

static int dp_state(const PftFilterAccess& a, PftDepthState** out) {
  if (!*a.depth) {
    PftDepthState* s = new PftDepthState();
    *a.depth = s;  // (freed with the handle whatever fails below)
    PFT_HIPCHK(&a, hipEventCreateWithFlags(&s->ev_up, hipEventDisableTiming));
    for (DpSlot& q : s->slot) PFT_HIPCHK(&a, hipEventCreateWithFlags(&q.ev, hipEventDisableTiming));
  }
  *out = *a.depth;
  return PFT_OK;
}

// a device image of at least `bytes` + DP_PAD; growing drains the stream first (an earlier kernel may still read the old one)
static int dp_reserve(const PftFilterAccess& a, uint8_t** p, size_t* cap, size_t bytes) {
  if (bytes + DP_PAD <= *cap) return PFT_OK;
  PFT_HIPCHK(&a, hipStreamSynchronize(a.stream));
  pft_dfree(*p);
  *cap = 0;
  PFT_HIPCHK(&a, pft_dalloc(p, bytes + DP_PAD));
  *cap = bytes + DP_PAD;
  return PFT_OK;
}

static int dp_apply(pft_filter* f, const pft_depth_frame* d, const void* depth, const void* color, bool wait) {
  if (!f) return PFT_ERR_INVALID_ARG;
  const PftFilterAccess a = pftf_access(f);
  DpLayout L;
  int r = dp_validate(d, &a.err, &L);
  if (r != PFT_OK) return r;
  if (!depth) return dp_invalid(&a.err, "depth", "pointer is null");
  if (d->color_format != PFT_COLOR_NONE && !color) return dp_invalid(&a.err, "color", "pointer is missing while color_format is set");
  PFT_HIPCHK(&a, hipSetDevice(a.device_id));
  PftDepthState* s = nullptr;
  r = dp_state(a, &s);
  if (r != PFT_OK) return r;
  r = dp_reserve(a, &s->d_depth, &s->cap_depth, L.depth_bytes);
  if (r != PFT_OK) return r;
  if (L.color_bytes) {
    r = dp_reserve(a, &s->d_color, &s->cap_color, L.color_bytes);
    if (r != PFT_OK) return r;
  }
  pft_point_xyzrgba* d_in = nullptr;
  r = pftf_begin_own_input(f, L.n, &d_in);
  if (r != PFT_OK) return r;
  // pointers of a pinned slot: nothing of the caller's is borrowed beyond the slot's own rule
  DpSlot* slot = nullptr;
  for (DpSlot& q : s->slot)
    if (q.depth && depth == q.depth && (!L.color_bytes || color == q.color) && L.depth_bytes <= q.depth_bytes &&
        L.color_bytes <= q.color_bytes)
      slot = &q;
  if (slot && slot->recorded) PFT_HIPCHK(&a, hipEventSynchronize(slot->ev));  // a busy slot: its earlier upload first
  PFT_HIPCHK(&a, hipMemcpyAsync(s->d_depth, depth, L.depth_bytes, hipMemcpyHostToDevice, a.stream));
  if (L.color_bytes) PFT_HIPCHK(&a, hipMemcpyAsync(s->d_color, color, L.color_bytes, hipMemcpyHostToDevice, a.stream));
  if (slot) {
    PFT_HIPCHK(&a, hipEventRecord(slot->ev, a.stream));
    slot->recorded = true;
  } else {
    PFT_HIPCHK(&a, hipEventRecord(s->ev_up, a.stream));
  }
  DpParams p;
  p.n = (uint32_t)L.n;
  p.W = (uint32_t)d->width;
  p.ifx = 1.0f / d->fx;
  p.ify = 1.0f / d->fy;
  p.cx = d->cx;
  p.cy = d->cy;
  p.divisor = d->depth_divisor;
  p.depth_format = d->depth_format;
  p.color_format = d->color_format;
  p.depth_stride = L.depth_stride;
  p.color_stride = L.color_stride;
  p.depth_aligned = L.depth_stride % dp_depth_bpp(d->depth_format) == 0;
  p.color_aligned = L.color_stride % 4u == 0;
  hipLaunchKernelGGL(k_depth_deproject, dim3((uint32_t)((L.n + DP_THREADS - 1) / DP_THREADS)), dim3(DP_THREADS), 0, a.stream,
                     p, s->d_depth, s->d_color, d_in);
  PFT_HIPCHK(&a, hipGetLastError());
  r = pftf_run_own_input(f, L.n, wait);
  if (r != PFT_OK) return r;
  if (!wait && !slot) PFT_HIPCHK(&a, hipEventSynchronize(s->ev_up));  // the caller's images are only borrowed for this call
  return PFT_OK;
}

extern "C" void pft_depth_frame_default(pft_depth_frame* d) {
  if (!d) return;
  memset(d, 0, sizeof(*d));
  d->abi_version = PFT_ABI_VERSION;
  d->width = 960;  // Kinect2 qhd, auto_tracking.cpp:775
  d->height = 540;
  d->fx = d->fy = 540.0f;
  d->cx = 479.5f;
  d->cy = 269.5f;
  d->depth_format = PFT_DEPTH_U16;
  d->depth_divisor = 1000.0f;
  d->color_format = PFT_COLOR_BGR8;
}

extern "C" int pft_filter_apply_depth(pft_filter* f, const pft_depth_frame* d, const void* depth, const void* color) {
  return dp_apply(f, d, depth, color, true);
}

extern "C" int pft_filter_apply_depth_async(pft_filter* f, const pft_depth_frame* d, const void* depth, const void* color) {
  return dp_apply(f, d, depth, color, false);
}

extern "C" int pft_filter_depth_host_buffers(pft_filter* f, const pft_depth_frame* d, int slot, void** depth, void** color) {
  if (!f || !depth || !color) return PFT_ERR_INVALID_ARG;
  const PftFilterAccess a = pftf_access(f);
  if (slot < 0 || slot >= PFT_DEPTH_SLOTS) return dp_invalid(&a.err, "slot", "is not 0 .. PFT_DEPTH_SLOTS - 1");
  DpLayout L;
  int r = dp_validate(d, &a.err, &L);
  if (r != PFT_OK) return r;
  PFT_HIPCHK(&a, hipSetDevice(a.device_id));
  PftDepthState* s = nullptr;
  r = dp_state(a, &s);
  if (r != PFT_OK) return r;
  DpSlot& q = s->slot[slot];
  // a full last row, so that a slot serves every stride of the description it was asked for
  const size_t need_d = (size_t)d->height * L.depth_stride, need_c = (size_t)d->height * L.color_stride;
  if (need_d > q.depth_bytes || need_c > q.color_bytes) {
    if (q.recorded) PFT_HIPCHK(&a, hipEventSynchronize(q.ev));
    q.recorded = false;
    if (need_d > q.depth_bytes) {
      if (q.depth) PFT_HIPCHK(&a, hipHostFree(q.depth));
      q.depth = nullptr;
      q.depth_bytes = 0;
      PFT_HIPCHK(&a, hipHostMalloc(&q.depth, need_d, hipHostMallocDefault));
      q.depth_bytes = need_d;
    }
    if (need_c > q.color_bytes) {
      if (q.color) PFT_HIPCHK(&a, hipHostFree(q.color));
      q.color = nullptr;
      q.color_bytes = 0;
      PFT_HIPCHK(&a, hipHostMalloc(&q.color, need_c, hipHostMallocDefault));
      q.color_bytes = need_c;
    }
  }
  *depth = q.depth;
  *color = d->color_format == PFT_COLOR_NONE ? nullptr : q.color;
  return PFT_OK;
}

extern "C" int pft_filter_depth_slot_done(pft_filter* f, int slot, int wait, int* done) {
  if (!f || !done) return PFT_ERR_INVALID_ARG;
  const PftFilterAccess a = pftf_access(f);
  if (slot < 0 || slot >= PFT_DEPTH_SLOTS) return dp_invalid(&a.err, "slot", "is not 0 .. PFT_DEPTH_SLOTS - 1");
  PftDepthState* s = *a.depth;
  if (!s || !s->slot[slot].recorded) {  // never used (or its upload already waited for): nothing in flight
    *done = 1;
    return PFT_OK;
  }
  PFT_HIPCHK(&a, hipSetDevice(a.device_id));
  DpSlot& q = s->slot[slot];
  if (wait) {
    PFT_HIPCHK(&a, hipEventSynchronize(q.ev));
    q.recorded = false;
    *done = 1;
    return PFT_OK;
  }
  const hipError_t e = hipEventQuery(q.ev);
  if (e == hipSuccess) {
    q.recorded = false;
    *done = 1;
  } else if (e == hipErrorNotReady) {
    *done = 0;
  } else {
    PFT_HIPCHK(&a, e);
  }
  return PFT_OK;
}
