// sr_api.hip -- host side of libspectrobot_hip.so: the C ABI of
// include/spectrobot_hip.h on top of the launchers of sr_kernels.hpp (the coefficient op: sr_kernels.hip, the limb
// family: sr_limb.hip and the state units, the small operators: sr_ops.hip, the solar source: sr_solar_source.hip).
//
// Host work is limited to what the reference also does once per call in plain
// Python: line filtering / window centres (spect_classes.py:1384-1388, 1937-1943),
// per-layer scalars and level populations (spect_main_module.py:2049-2073),
// TIPS-2003 lookup + 4-point Lagrange (spect_classes.py:1680-1710).  Every
// per-(line, layer) and per-grid-point quantity is computed on the GPU; there is
// no CPU fallback for any of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/spectrobot_hip.h"
#include "sr_kernels.hpp"
#include "sr_solar_plan.hpp"
#include "tips2003_tables.inc"

using namespace sr;

namespace {

thread_local std::string g_err;

int hip_fail(hipError_t e, const char *what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return SR_ERR_HIP;
}
#define HIPCHK(expr)                                  \
  do {                                                \
    hipError_t e__ = (expr);                          \
    if (e__ != hipSuccess) return hip_fail(e__, #expr); \
  } while (0)
#define LAUNCHCHK(expr)                                              \
  do {                                                               \
    int e__ = (expr);                                                \
    if (e__ != 0) return hip_fail((hipError_t)e__, "kernel launch"); \
  } while (0)

// Every stream the library makes or destroys goes through these two: sr_stream_census reports their counts.
std::atomic<int> g_streams_live{0}, g_streams_total{0};
int stream_create(hipStream_t *s) {
  HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  ++g_streams_live;
  ++g_streams_total;
  return SR_OK;
}
void stream_destroy(hipStream_t &s) {
  if (!s) return;
  (void)hipStreamDestroy(s);
  s = nullptr;
  --g_streams_live;
}

// The ONE staging stream of this thread on device `dev` (Stager::push_early / begin_early): early host-to-device copies
// and the work that depends on them alone.  Thread-local, never destroyed; it is the third of the three streams the
// library keeps per (thread, device) beside a handle's two pipeline streams (CoefWork).
int staging_stream(int dev, hipStream_t *out) {
  static thread_local std::map<int, hipStream_t> streams; // one per device this thread has used
  hipStream_t &s = streams[dev];
  if (!s) {
    const int rc = stream_create(&s);
    if (rc) return rc;
  }
  *out = s;
  return SR_OK;
}

// grow-only device buffer
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  unsigned gen = 0; // bumped whenever the block is (re)allocated or released: what a cache of the CONTENTS keys on (a new
                    // block may come back at the old address)
  int ensure(size_t bytes) {
    if (bytes <= cap) return SR_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    ++gen;
    size_t want = bytes + bytes / 8 + 256;
    HIPCHK(hipMalloc(&p, want));
    cap = want;
    return SR_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    ++gen;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

// Pinned host staging buffer with a device mirror: fill host(), then push() on
// the caller's stream; the next prepare() waits for the previous copy only.
struct Stager {
  void *h = nullptr;
  size_t hcap = 0;
  DevBuf d;
  hipEvent_t done = nullptr;
  bool pending = false;
  int dev = -1; // device the mirror, the event and the pinned buffer belong to
  int prepare(size_t bytes) {
    // the thread-local rings outlive a hipSetDevice(): a slot made on another device is rebuilt on this one
    int cur = 0;
    HIPCHK(hipGetDevice(&cur));
    if (dev != cur) {
      if (dev >= 0) {
        HIPCHK(hipSetDevice(dev));
        release();
        HIPCHK(hipSetDevice(cur));
      }
      dev = cur;
    }
    if (pending) {
      HIPCHK(hipEventSynchronize(done));
      pending = false;
    }
    if (!done) HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    if (bytes > hcap) {
      if (h) (void)hipHostFree(h);
      h = nullptr;
      hcap = 0;
      const size_t want = bytes + bytes / 8 + 256;
      HIPCHK(hipHostMalloc(&h, want, hipHostMallocDefault));
      hcap = want;
    }
    return d.ensure(std::max<size_t>(bytes, 16));
  }
  int push(size_t bytes, hipStream_t st) {
    if (bytes) HIPCHK(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(done, st));
    pending = true;
    return SR_OK;
  }
  // The copy on the staging stream, `st` only waits for it.  Host-to-device copies of all streams
  // share the DMA queues in issue order: a small staging copy enqueued on `st` BEHIND 8 ms of kernels
  // held back the next call's layer-scalar copy (on the prep stream) and with it the pipelined
  // preparation of the next call's tables (+0.9 ms per step).  prepare() has already waited for the
  // slot's last consumers, so the copy may run at once.
  int push_early(size_t bytes, hipStream_t st) {
    hipStream_t copy_st = nullptr;
    const int rc = staging_stream(dev, &copy_st);
    if (rc) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, copy_st));
    HIPCHK(hipEventRecord(done, copy_st));
    HIPCHK(hipStreamWaitEvent(st, done, 0));
    pending = true;
    return SR_OK;
  }
  // push_early in two halves, for work that depends on the staged data alone (the LOS column integration): it runs
  // on the staging stream right behind the copy, i.e. as soon as the host has issued it -- on `st` it queued behind
  // everything the caller had submitted before (on a 1/8 shard: copy, columns kernel and two event hand-overs, ~35 us
  // of a 0.9 ms step, after the coefficient kernels instead of beside them).
  int begin_early(size_t bytes, hipStream_t *copy_stream_out) {
    hipStream_t cs = nullptr;
    const int rc = staging_stream(dev, &cs);
    if (rc) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, cs));
    *copy_stream_out = cs;
    return SR_OK;
  }
  int end_early(hipStream_t copy_stream, hipStream_t st) {
    HIPCHK(hipEventRecord(done, copy_stream));
    HIPCHK(hipStreamWaitEvent(st, done, 0));
    pending = true;
    return SR_OK;
  }
  // re-record `done` behind the kernels that read (or write) the device mirror, so that the slot is
  // not refilled while they run
  int mark(hipStream_t st) {
    HIPCHK(hipEventRecord(done, st));
    pending = true;
    return SR_OK;
  }
  void release() {
    if (pending && done) (void)hipEventSynchronize(done);
    pending = false;
    if (h) (void)hipHostFree(h);
    h = nullptr;
    hcap = 0;
    d.release();
    if (done) (void)hipEventDestroy(done);
    done = nullptr;
  }
  template <class T> T *host() const { return static_cast<T *>(h); }
};

// A call site's small ring of staging buffers (each site declares its own, static thread_local): reusing one buffer
// would make every call wait for the previous call's copy, i.e. for the GPU to reach it, and keep the host at most one
// step ahead; with four slots a call waits for the one four calls back.
struct StagerRing {
  Stager s[4];
  unsigned next = 0;
  Stager &take() { return s[next++ & 3]; }
};

// The layout of one staged block in a Stager: typed arrays one after the other, each on a 16-byte boundary, then an
// optional device-only tail.  Two phases: the parts are registered first (copy / zeros / room / tail); prepare() sizes
// the slot and fills the host side, after it host() and dev() give a part's two addresses and push_early() (or
// begin_early, then the slot's end_early) sends the host parts up.  An offset and the type read back from it are one
// Part<T>.
class StagePack {
 public:
  template <class T> struct Part { size_t off; };
  explicit StagePack(Stager &slot) : sg_(slot) {}
  Stager &slot() const { return sg_; } // for mark() and end_early()
  // n elements copied from src; `room` keeps a part that may be empty at least that many elements long
  template <class T> Part<T> copy(const T *src, size_t n, size_t room = 0) {
    return {place(src, sizeof(T) * n, sizeof(T) * std::max(n, room), false)};
  }
  template <class T> Part<T> zeros(size_t n) { return {place(nullptr, 0, sizeof(T) * n, true)}; }
  template <class T> Part<T> room(size_t n) { return {place(nullptr, 0, sizeof(T) * n, false)}; } // the caller fills host(part)
  void tail(size_t bytes) { tail_ = bytes; } // device only, behind the staged parts: never copied
  int prepare() {
    const int rc = sg_.prepare(in_bytes() + tail_);
    if (rc) return rc;
    for (int i = 0; i < n_; ++i) {
      if (it_[i].src && it_[i].bytes) std::memcpy(sg_.host<char>() + it_[i].off, it_[i].src, it_[i].bytes);
      if (it_[i].zero) std::memset(sg_.host<char>() + it_[i].off, 0, it_[i].bytes);
    }
    return SR_OK;
  }
  int push_early(hipStream_t st) { return sg_.push_early(in_bytes(), st); }
  int stage(hipStream_t st) { // prepare + push_early, for blocks without parts filled in place
    const int rc = prepare();
    return rc ? rc : push_early(st);
  }
  int begin_early(hipStream_t *copy_stream_out) { return sg_.begin_early(in_bytes(), copy_stream_out); }
  template <class T> T *host(Part<T> p) const { return reinterpret_cast<T *>(sg_.host<char>() + p.off); }
  template <class T> const T *dev(Part<T> p) const { return reinterpret_cast<const T *>(sg_.d.as<char>() + p.off); }
  template <class T> T *dev_tail() const { return reinterpret_cast<T *>(sg_.d.as<char>() + in_bytes()); }

 private:
  struct Item { size_t off, bytes; const void *src; bool zero; };
  static size_t al(size_t v) { return (v + 15) / 16 * 16; }
  size_t in_bytes() const { return al(end_); }
  size_t place(const void *src, size_t bytes, size_t room_bytes, bool zero) {
    if (n_ == kMaxParts) abort(); // (a programming error: raise kMaxParts)
    const size_t off = al(end_);
    it_[n_++] = Item{off, zero ? room_bytes : bytes, src, zero};
    end_ = off + room_bytes;
    return off;
  }
  static constexpr int kMaxParts = 12;
  Stager &sg_;
  Item it_[kMaxParts];
  int n_ = 0;
  size_t end_ = 0, tail_ = 0;
};

// ---- TIPS-2003 (fparts_mod.f:33-295) + CalcPartitionSum (spect_classes.py:1692-1710) ----
int tips_row(int mol, int iso) {
  for (int i = 0; i < kTipsNTab; ++i)
    if (kTipsKey[i][0] == mol && kTipsKey[i][1] == iso) return i;
  return -1;
}

// scipy.interpolate.lagrange through the two table points <= T and the two > T:
// polynomial assembled in coefficient form by successive products with
// (x - x_k)/(x_j - x_k), summed, then evaluated by Horner -- the order of
// operations of scipy's poly1d arithmetic, which the result depends on at 1e-13.
double lagrange4(const double *tg, const double *qg, int n, double temp) {
  double xs[4], qs[4];
  int m = 0, n_le = 0;
  while (n_le < n && tg[n_le] <= temp) ++n_le;
  for (int i = std::max(0, n_le - 2); i < n_le; ++i, ++m) { xs[m] = tg[i]; qs[m] = qg[i]; }
  for (int i = n_le; i < std::min(n, n_le + 2); ++i, ++m) { xs[m] = tg[i]; qs[m] = qg[i]; }
  std::vector<double> poly(1, 0.0);
  for (int j = 0; j < m; ++j) {
    std::vector<double> pt(1, qs[j]);
    for (int k = 0; k < m; ++k) {
      if (k == j) continue;
      const double fac = xs[j] - xs[k];
      const double f0 = 1.0 / fac, f1 = -xs[k] / fac;
      std::vector<double> nx(pt.size() + 1, 0.0);
      for (size_t i = 0; i < nx.size(); ++i) {
        double s = 0.0;
        if (i < pt.size()) s += pt[i] * f0;
        if (i >= 1) s += pt[i - 1] * f1;
        nx[i] = s;
      }
      pt.swap(nx);
    }
    if (pt.size() > poly.size()) poly.insert(poly.begin(), pt.size() - poly.size(), 0.0);
    const size_t off = poly.size() - pt.size();
    for (size_t i = 0; i < pt.size(); ++i) poly[off + i] += pt[i];
  }
  double y = 0.0;
  for (double c : poly) y = y * temp + c;
  return y;
}

// Host copy of a (filtered, centre-sorted) line list in the layout of the device SoA: 12 double
// arrays then 3 int arrays of length md.
struct HostLines {
  size_t md = 1;   // array stride (>= 1)
  int64_t m = 0;   // lines
  std::vector<double> d;
  std::vector<int> i;
  std::vector<double> p_shift, self_broad; // sr_lineset_set_line_shape: [md] each, or empty (unset)
};

// Process-wide mode switches (sr_set_*).  Atomic: a call reads each ONCE at entry and works with that
// snapshot, so flipping a switch from another thread never changes a call half way.
std::atomic<int> g_variant{8};   // points per lane in the exact wings kernel
std::atomic<int> g_far_field{3}; // 1: far wings by per-line local expansions, 2: by box pairs (multipole -> local), 3 (default): 2, but sparse line sets by 1, 0: every evaluation exact
std::atomic<int> g_overlap{1};   // 1 (default): the decoupled, phased pipeline; 0: kernels one after the other
// sr_set_jac_layer_mode; SR_JAC_LAYER_MODE (environment, read once at load): its initial value, for A/B runs of whole programs
std::atomic<int> g_band_fusion{1}; // sr_set_band_fusion
std::atomic<int> g_state_ray_blocks{0}; // sr_set_state_ray_blocks
std::atomic<int> g_jac_layer_forward{[] { const char *e = getenv("SR_JAC_LAYER_MODE"); const int v = e ? atoi(e) : 0; return v >= 0 && v <= 3 ? v : 0; }()};
// sr_set_kernel_repeat: a measurement hook of the SERIAL schedule -- kernel g_repeat_kernel of every call is launched
// g_repeat_n times back to back (energy per launch: tools/energy_by_kernel.py loops one kernel for seconds beside a power
// sampler).  0 prep, 1 level-0 far-field pass, 2 S2M + M2M, 3 M2L, 4 zones, 5 wings.  Results of a repeated M2L are NOT
// valid (it adds into the level-0 coefficients); everything else stores.
std::atomic<int> g_repeat_kernel{-1}, g_repeat_n{1};
std::atomic<int> g_level_route{1}; // sr_set_level_route: 1 (default) the multi-channel pass for level tables, 0 one coefficient op per level
std::atomic<int> g_timing{1};    // 0: no timing events in the coefficient op (sr_set_timing: seven hipEventRecord fewer per call)
std::atomic<int> g_counting{0};  // 1: counting instantiations of the far-field-mode kernels (sr_set_counting)
std::atomic<size_t> g_table_budget{(size_t)48 << 30}; // bytes of FastRec + ColdRec tables per layer batch

} // namespace

// Per-call scratch and stream / event state of the coefficient op.  A lineset owns one; the per-level sub-linesets
// (level_set) SHARE their parent's -- calls on a handle and its children are serialised through ev_last_done anyway,
// and twelve levels with their own record tables, far-field scratch, streams and events held twelve times the memory.
struct CoefWork {
  // [2]: with sr_set_overlap(1) the tables of call c+1 are prepared (on far_st) while the kernels
  // of call c still read theirs
  Stager s_layers[2];
  DevBuf d_fast[2], d_cold[2], d_coef[2], d_zone2[2], d_mom[2], d_outer_recs;
  // The TWO internal streams of the pipelined schedule.  On each, stream order IS the order the phased schedule runs
  // its kernels in anyway, so the pair (with the caller's stream) needs three hardware queues, not six:
  //   far_st:  staging copy + prep(c) -> level-0 pass(c) -> S2M, M2M(c) -> M2L(c) [-> L2L, far-only passes] -> prep(c + 1) ..
  //   near_st: zones(c), gated by an event behind the level-0 pass and S2M of its own call
  // (the wings kernel, which writes the caller-visible output, is on the caller's stream).
  // streams_of: the CoefWork whose pair this one runs on -- the private CoefWorks of a multi-channel pass (McWork::fw)
  // borrow the handle's; the owner creates the pair on first use and is the only one that destroys it.
  hipStream_t far_st = nullptr, near_st = nullptr;
  CoefWork *streams_of = nullptr;
  hipEvent_t ev_prep_done[2] = {nullptr, nullptr}, ev_tables_free[2] = {nullptr, nullptr}, ev_op0 = nullptr;
  // the far-field chain (level-0 pass, moments, upward pass, translations) of call c + 1 runs on far_st behind its
  // table preparation, i.e. beside the zones / wings kernels of call c (its own coefficient / moment buffers)
  hipEvent_t ev_far_done[2] = {nullptr, nullptr}, ev_zones_done[2] = {nullptr, nullptr};
  hipEvent_t ev_s2m_done[2] = {nullptr, nullptr}; // behind S2M + M2M: what releases the zones kernel (box-pair mode)
  bool free_recorded[2] = {false, false};
  int parity = 0;
  bool overlapped = false;       // last call ran that way (timing hook)
  bool pipelined = false;        // last call prepared its tables on far_st
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int n_timed = 0; // kernels timed in the last call
  bool timed = false;
  // d_coef / d_counts and (without overlap) the single table set are shared by consecutive
  // calls: every call first makes its streams wait for the end of the previous call on this handle,
  // whatever stream that one ran on (ev_last_done), so calls on unrelated caller streams are safe.
  hipEvent_t ev_last_done = nullptr;
  bool last_done_recorded = false;
  DevBuf d_counts; // kCntN executed-work counters of the last counting call
  bool counted = false;
  int init() {
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventCreateWithFlags(&ev_last_done, hipEventDisableTiming));
    return SR_OK;
  }
  // the events of the pipelined schedule, on its first call
  int pipeline_events() {
    if (ev_op0) return SR_OK;
    HIPCHK(hipEventCreateWithFlags(&ev_op0, hipEventDefault));
    for (int i = 0; i < 2; ++i) {
      HIPCHK(hipEventCreateWithFlags(&ev_prep_done[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_tables_free[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_far_done[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_zones_done[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_s2m_done[i], hipEventDisableTiming));
    }
    return SR_OK;
  }
  // The end of a call whose last kernel went to `st`: table set b (-1: none read) is free behind it, where the
  // pipeline's events exist, and the next call on the handle waits for ev_last_done
  int end_call(hipStream_t st, int b) {
    if (b >= 0 && ev_tables_free[b]) {
      HIPCHK(hipEventRecord(ev_tables_free[b], st));
      free_recorded[b] = true;
    }
    HIPCHK(hipEventRecord(ev_last_done, st));
    last_done_recorded = true;
    return SR_OK;
  }
  int pipeline_streams(hipStream_t *far, hipStream_t *near) {
    CoefWork &o = streams_of ? *streams_of : *this;
    if (!o.far_st) { // (each on its own: a pair half made by a failed call is completed by the next, never handed out)
      const int rc = stream_create(&o.far_st);
      if (rc) return rc;
    }
    if (!o.near_st) {
      const int rc = stream_create(&o.near_st);
      if (rc) return rc;
    }
    *far = o.far_st;
    *near = o.near_st;
    return SR_OK;
  }
  void release() {
    for (int b = 0; b < 2; ++b) {
      s_layers[b].release();
      d_fast[b].release();
      d_cold[b].release();
      if (ev_prep_done[b]) (void)hipEventDestroy(ev_prep_done[b]);
      if (ev_tables_free[b]) (void)hipEventDestroy(ev_tables_free[b]);
      if (ev_far_done[b]) (void)hipEventDestroy(ev_far_done[b]);
      if (ev_zones_done[b]) (void)hipEventDestroy(ev_zones_done[b]);
      if (ev_s2m_done[b]) (void)hipEventDestroy(ev_s2m_done[b]);
      d_zone2[b].release();
      d_coef[b].release();
      d_mom[b].release();
    }
    if (ev_op0) (void)hipEventDestroy(ev_op0);
    if (ev_last_done) (void)hipEventDestroy(ev_last_done);
    d_counts.release();
    d_outer_recs.release();
    stream_destroy(far_st); // (its own pair: a borrowed one, streams_of, is the owner's to destroy)
    stream_destroy(near_st);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Scratch of the multi-channel pass (mc_pass): record tables of the FULL list with the three channel weights, the
// far-only coefficients of the level passes, and the CoefWorks the far-only passes run through (not the handle's shared
// one: folded ops on the handle and the passes of one table build do not wait for each other's scratch).  It makes no
// streams: the sparse batch runs on the handle's near_st, the dense passes' chains on its far_st (CoefWork::streams_of).
// kMcFarLanes: CoefWorks the dense far-only level passes rotate through (tables, events; the handle's streams).  They
// run one after the other on far_st, so the lanes buy no concurrency any more, only that a pass prepares its tables
// without waiting for the one before it to finish with a shared set: two CoefWorks x two parities cover the one or two
// dense passes of a build (it was four when each lane had streams of its own).
constexpr int kMcFarLanes = 2;
struct McWork {
  CoefWork fw[kMcFarLanes];
  bool fw_init = false, batch_pending = false;
  Stager s_layers, s_far, s_batch;
  DevBuf d_fast, d_cold, d_coef, d_outer_recs, d_bfast;
  hipEvent_t ev_prep = nullptr, ev_zones = nullptr;
  hipEvent_t ev_t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; // timing: start, after the tables, after the zones kernel, before / after the wings kernel
  bool timed = false;
  void release() {
    if (fw_init)
      for (auto &f : fw) f.release();
    fw_init = false;
    s_layers.release();
    s_far.release();
    s_batch.release();
    d_fast.release();
    d_cold.release();
    d_coef.release();
    d_outer_recs.release();
    d_bfast.release();
    if (ev_prep) (void)hipEventDestroy(ev_prep);
    if (ev_zones) (void)hipEventDestroy(ev_zones);
    for (auto &e : ev_t)
      if (e) { (void)hipEventDestroy(e); e = nullptr; }
    ev_prep = ev_zones = nullptr;
  }
};

struct sr_lineset {
  int64_t n_lines = 0; // main lines (centre inside its own window)
  HostLines host, host_outer; // host copies: per-level subsets are cut from them (level_set)
  int n_outer = 0;            // lines whose centre lies outside their window (outer branches)
  DevBuf d_lines_outer;
  LinesDev Lo{};
  // per-level sub-linesets (lines whose upper or lower level is L), built on first use by the
  // G-coefficient / tracked-level entry points; nullptr until then
  std::vector<sr_lineset *> level_sets;
  std::vector<sr_lineset *> level_up_sets; // the lines whose UPPER level is L only (the ind_emission pass)
  DevBuf d_gscratch;          // second output channel of the ind_emission pass
  GridParams gp{};
  int mol = 0, iso = 0, n_levels = 0;
  double mm = 0.0;
  std::vector<double> e_lev;
  std::vector<int> ic; // host copy, sorted
  double freq_max = 0.0;
  double gamma_max = 0.0, ndep_min = 0.0, ndep_max = 0.0; // air (and self) broadening / its temperature exponent over the lines
  double shift_max = 0.0;           // sr_lineset_set_line_shape: largest |p_shift| over the lines, cm^-1 / atm (0: unset)
  std::vector<double> self_press;   // sr_lineset_set_self_pressure: hPa per layer of the next calls; empty = 0
  int64_t n_disp_lo = 0, n_disp_hi = 0; // leading / trailing lines centred beyond the grid ends (window clamped to the end point)
  DevBuf d_lines;      // one allocation, carved below
  LinesDev L{};
  DevBuf d_first;
  int first_x0 = 0, first_n = 0; // IcIndex table domain
  CoefWork own_work;
  CoefWork *work = nullptr;      // &own_work, or the parent's for a per-level sub-lineset
  McWork mc;                     // the multi-channel pass of this handle (parents only)
  std::vector<double> bounds_temps; // sr_lineset_set_bounds_temps: empty = boundaries at the call's own temperatures
  sr_lineset *parent = nullptr;     // per-level sub-lineset: the handle it was cut from (its bounds_temps apply)
  bool linear_weights = false;      // sr_lineset_set_linear_weights (takes effect with bounds_temps only)
  // where every line came from: n_in lines were given to sr_lineset_create; in_main / in_outer: the input index of
  // each main / outer line (device order); d_inpos [n_in]: main position p, -2 - outer position, or -1 (filtered out)
  int64_t n_in = 0;
  std::vector<int64_t> in_main, in_outer;
  DevBuf d_inpos;
  // sr_lineset_set_strengths: HITRAN intensities in device order (main lines, then the outer ones) -- L.s_ref, Lo.s_ref
  DevBuf d_sref;
  bool has_strengths = false;
  double s_t_ref = 0.0, s_q_ref = 0.0, s_iso_ab = 1.0; // their temperature, Q there (<= 0: the TIPS tables), abundance
  Stager s_str;                                         // layer stage of sr_line_strengths_dev
};

extern "C" {

const char *sr_strerror(int s) {
  switch (s) {
    case SR_OK: return "ok";
    case SR_ERR_ARG: return "bad argument";
    case SR_ERR_LIMIT: return "size limit exceeded";
    case SR_ERR_HIP: return "HIP runtime error";
    case SR_ERR_NODEVICE: return "no gfx950 device";
    case SR_ERR_UNSUPPORTED: return "unsupported input";
    case SR_ERR_TABLE: return "(mol, iso) not in TIPS-2003 tables";
    default: return "unknown status";
  }
}
const char *sr_last_error(void) { return g_err.c_str(); }
int sr_abi_version(void) { return 1; }

int sr_set_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_err = "no HIP device visible";
    return SR_ERR_NODEVICE;
  }
  if (device < 0 || device >= n) return SR_ERR_ARG;
  HIPCHK(hipSetDevice(device));
  return SR_OK;
}

int sr_device_info(char *name, int name_len, int *cu_count, double *hbm_gib) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return SR_ERR_NODEVICE;
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, dev));
  if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (hbm_gib) *hbm_gib = (double)p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0);
  return SR_OK;
}

int sr_recommended_hw_queues(int *recommended, int *configured) {
  // 8: headroom for processes with several top-level linesets in flight (two pipeline streams each) or streams of their
  // own.  ONE handle needs no more than the runtime's default 4: caller + far_st + near_st + the staging stream.
  if (recommended) *recommended = 8;
  if (configured) {
    const char *e = getenv("GPU_MAX_HW_QUEUES");
    const int v = e ? atoi(e) : 0;
    *configured = v > 0 ? v : 4; // the runtime's default
  }
  return SR_OK;
}

int sr_stream_census(int *live, int *created_total) {
  if (live) *live = g_streams_live.load();
  if (created_total) *created_total = g_streams_total.load();
  return SR_OK;
}

int sr_set_table_budget(int64_t bytes) {
  if (bytes < (int64_t)(sizeof(FastRec) + sizeof(ColdRec))) return SR_ERR_ARG;
  g_table_budget.store((size_t)bytes);
  return SR_OK;
}

int sr_set_far_field(int on) {
  g_far_field.store(on < 0 ? 0 : (on > 3 ? 3 : on));
  return SR_OK;
}

int sr_set_overlap(int on) {
  g_overlap.store(on != 0 ? 1 : 0); // see spectrobot_hip.h
  return SR_OK;
}

int sr_set_kernel_repeat(int kernel, int n) {
  if (kernel < -1 || kernel > 5 || n < 1) return SR_ERR_ARG;
  g_repeat_kernel.store(kernel);
  g_repeat_n.store(kernel < 0 ? 1 : n);
  return SR_OK;
}

int sr_set_level_route(int multi_channel) {
  g_level_route.store(multi_channel ? 1 : 0);
  return SR_OK;
}

int sr_set_timing(int on) {
  g_timing.store(on == 2 ? 2 : (on ? 1 : 0));
  return SR_OK;
}

int sr_set_counting(int on) {
  g_counting.store(on ? 1 : 0);
  return SR_OK;
}

int sr_set_jac_layer_mode(int forward) {
  g_jac_layer_forward.store(forward == 2 || forward == 3 ? forward : (forward ? 1 : 0)); // see spectrobot_hip.h
  return SR_OK;
}

double sr_far_field_truncation_bound(void) { return 18.0 * std::pow((double)kTheta, -(double)(kFD + 1)); }

double sr_far_field_min_distance(int level, int pole_margin) {
  if (level < 0 || level >= kMaxFarLevels || pole_margin < 0 || pole_margin > (1 << 24)) return -1.0;
  return 0.5 * (double)ff_thr2(level, pole_margin); // the kernels' own threshold (sr_kernels.hpp)
}

int sr_set_band_fusion(int on) {
  g_band_fusion.store(on ? 1 : 0);
  return SR_OK;
}

int sr_limb_max_gases(int folded) { return folded ? kFoldGasMax : kLimbGasMax; }

int sr_set_state_ray_blocks(int on) {
  g_state_ray_blocks.store(on ? 1 : 0);
  return SR_OK;
}

// ray_jac_plan on the host, for tests and tools: no device, no stream
int sr_state_ray_plan(const sr_los_desc *los, int n_layers, int n_col, const int32_t *par_gas, const double *par_w, int n_lev,
                      const int32_t *par_lgas, const int32_t *par_level, const double *par_c, int n_row, const double *par_t,
                      int n_hid, int32_t *sizes4, int32_t *ray_blk_off, int32_t *blk, int32_t *col_row, int32_t *ent_off,
                      int32_t *slot_par, int32_t *ent_slot, int32_t *ent_level, double *ent_c) {
  LosShape shape;
  if (!sizes4 || n_layers <= 0 || n_lev < 0 || n_row < 0 || n_hid < 0) return SR_ERR_ARG;
  if (n_hid > (los && los->n_gas > kFoldGasMax ? kLimbGasMax : kFoldGasMax)) return SR_ERR_ARG; // (a hidden slot per gas)
  if ((n_lev > 0 && (!par_level || !par_c)) || (n_row > 0 && !par_t)) return SR_ERR_ARG;
  const int rc = check_los_par(los, n_layers, n_col, par_gas, par_w, &shape, kLimbGasMax);
  if (rc) return rc;
  const RayJacPlan R = ray_jac_plan(los, n_col, par_gas, par_w, n_lev, par_level, par_c, n_layers, n_row, par_t, par_lgas, n_hid,
                                    state_gas_bits(los->n_gas));
  sizes4[0] = R.np, sizes4[1] = R.n_blocks, sizes4[2] = R.ray_blk_off.back(), sizes4[3] = (int32_t)R.ent.size();
  if (ray_blk_off) std::copy(R.ray_blk_off.begin(), R.ray_blk_off.end(), ray_blk_off);
  if (blk) std::copy(R.blk.begin(), R.blk.end(), blk);
  if (col_row) std::copy(R.col_row.begin(), R.col_row.end(), col_row);
  if (ent_off) std::copy(R.ent_off.begin(), R.ent_off.end(), ent_off);
  if (slot_par) std::copy(R.slot_par.begin(), R.slot_par.end(), slot_par);
  for (size_t i = 0; i < R.ent.size(); ++i) {
    if (ent_slot) ent_slot[i] = R.ent[i].slot;
    if (ent_level) ent_level[i] = R.ent[i].level;
    if (ent_c) ent_c[i] = R.ent[i].c;
  }
  return SR_OK;
}

int sr_set_points_per_lane(int p) {
  if (p != 4 && p != 8) return SR_ERR_ARG;
  g_variant.store(p);
  return SR_OK;
}

// ------------------------------------------------------------------------
int sr_bd_tips_2003(int mol, int iso, double *gi, double *t_grid119, double *qt_grid119) {
  const int r = tips_row(mol, iso);
  if (r < 0) return SR_ERR_TABLE;
  if (gi) *gi = kTipsGi[r];
  if (t_grid119) std::memcpy(t_grid119, kTipsT, sizeof(double) * kTipsNT);
  if (qt_grid119) std::memcpy(qt_grid119, kTipsQ[r], sizeof(double) * kTipsNT);
  return SR_OK;
}

int sr_calc_partition_sum(int mol, int iso, const double *temps, int n, double *q_out) {
  if (!temps || !q_out || n < 0) return SR_ERR_ARG;
  const int r = tips_row(mol, iso);
  if (r < 0) return SR_ERR_TABLE;
  for (int i = 0; i < n; ++i) q_out[i] = lagrange4(kTipsT, kTipsQ[r], kTipsNT, temps[i]);
  return SR_OK;
}

} // extern "C"

// ------------------------------------------------------------------------
namespace {

int upload_soa(const HostLines &H, DevBuf &buf, LinesDev &L) {
  const size_t bytes_d = H.d.size() * sizeof(double), bytes_i = H.i.size() * sizeof(int);
  // the line-shape arrays, when set, behind the int arrays (at a multiple of 8 bytes)
  const size_t off_x = bytes_d + (bytes_i + 7) / 8 * 8, bytes_x = H.md * sizeof(double);
  int rc = buf.ensure(off_x + 2 * bytes_x);
  if (rc) return rc;
  char *base = buf.as<char>();
  HIPCHK(hipMemcpy(base, H.d.data(), bytes_d, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(base + bytes_d, H.i.data(), bytes_i, hipMemcpyHostToDevice));
  L.p_shift = L.self_broad = nullptr;
  if (!H.p_shift.empty()) {
    HIPCHK(hipMemcpy(base + off_x, H.p_shift.data(), bytes_x, hipMemcpyHostToDevice));
    L.p_shift = reinterpret_cast<const double *>(base + off_x);
  }
  if (!H.self_broad.empty()) {
    HIPCHK(hipMemcpy(base + off_x + bytes_x, H.self_broad.data(), bytes_x, hipMemcpyHostToDevice));
    L.self_broad = reinterpret_cast<const double *>(base + off_x + bytes_x);
  }
  const double *dd = reinterpret_cast<const double *>(base);
  const int *di = reinterpret_cast<const int *>(base + bytes_d);
  const size_t md = H.md;
  L.freq = dd + 0 * md; L.hcf = dd + 1 * md; L.a_coeff = dd + 2 * md; L.b21 = dd + 3 * md;
  L.b12 = dd + 4 * md; L.e_lower = dd + 5 * md; L.g_up = dd + 6 * md; L.g_lo = dd + 7 * md;
  L.air_broad = dd + 8 * md; L.t_dep = dd + 9 * md; L.evib_up = dd + 10 * md; L.evib_lo = dd + 11 * md;
  L.ic = di + 0 * md; L.lev_up = di + 1 * md; L.lev_lo = di + 2 * md;
  L.n_lines = (int)H.m;
  return SR_OK;
}

// rows `sel` of H (ascending, so the subset stays sorted by window centre)
HostLines subset(const HostLines &H, const std::vector<int64_t> &sel) {
  HostLines S;
  S.m = (int64_t)sel.size();
  S.md = (size_t)std::max<int64_t>(S.m, 1);
  S.d.assign(12 * S.md, 0.0);
  S.i.assign(3 * S.md, 0);
  for (int64_t q = 0; q < S.m; ++q) {
    for (int a = 0; a < 12; ++a) S.d[a * S.md + q] = H.d[a * H.md + sel[q]];
    for (int a = 0; a < 3; ++a) S.i[a * S.md + q] = H.i[a * H.md + sel[q]];
  }
  if (!H.p_shift.empty()) {
    S.p_shift.assign(S.md, 0.0);
    for (int64_t q = 0; q < S.m; ++q) S.p_shift[q] = H.p_shift[sel[q]];
  }
  if (!H.self_broad.empty()) {
    S.self_broad.assign(S.md, 0.0);
    for (int64_t q = 0; q < S.m; ++q) S.self_broad[q] = H.self_broad[sel[q]];
  }
  return S;
}

} // namespace

// Device side of a lineset from its host line lists (main: centre inside its window; outer: not).
static int lineset_upload(sr_lineset *ls) {
  const HostLines &H = ls->host;
  ls->n_lines = H.m;
  ls->ic.assign(H.i.begin(), H.i.begin() + H.m);
  ls->freq_max = 0.0;
  for (int64_t q = 0; q < H.m; ++q) ls->freq_max = std::max(ls->freq_max, H.d[q]);
  for (int64_t q = 0; q < ls->host_outer.m; ++q) ls->freq_max = std::max(ls->freq_max, ls->host_outer.d[q]);
  ls->gamma_max = 0.0;
  ls->ndep_min = ls->ndep_max = H.m > 0 ? H.d[9 * H.md] : 0.0;
  for (int64_t q = 0; q < H.m; ++q) {
    ls->gamma_max = std::max(ls->gamma_max, H.d[8 * H.md + q]);
    ls->ndep_min = std::min(ls->ndep_min, H.d[9 * H.md + q]);
    ls->ndep_max = std::max(ls->ndep_max, H.d[9 * H.md + q]);
  }
  // sr_lineset_set_line_shape: lw <= (296/T)^n max(gamma_air, gamma_self) P for 0 <= Ps <= P; the largest |shift| over
  // main and outer lines
  if (!H.self_broad.empty())
    for (int64_t q = 0; q < H.m; ++q) ls->gamma_max = std::max(ls->gamma_max, H.self_broad[q]);
  ls->shift_max = 0.0;
  for (const HostLines *S : {&H, static_cast<const HostLines *>(&ls->host_outer)})
    for (int64_t q = 0; q < S->m && !S->p_shift.empty(); ++q) ls->shift_max = std::max(ls->shift_max, std::fabs(S->p_shift[q]));
  ls->n_disp_lo = ls->n_disp_hi = 0;
  if (H.m > 0) {
    const double g0 = grid_at(ls->gp, 0), g1 = grid_at(ls->gp, (int)ls->gp.n_grid - 1), tol = 0.75 * ls->gp.gstep;
    while (ls->n_disp_lo < H.m && H.i[ls->n_disp_lo] == 0 && H.d[ls->n_disp_lo] < g0 - tol) ++ls->n_disp_lo;
    while (ls->n_disp_hi < H.m - ls->n_disp_lo && H.i[H.m - 1 - ls->n_disp_hi] == (int)ls->gp.n_grid - 1 &&
           H.d[H.m - 1 - ls->n_disp_hi] > g1 + tol)
      ++ls->n_disp_hi;
  }
  int rc = upload_soa(H, ls->d_lines, ls->L);
  if (rc) return rc;
  ls->n_outer = (int)ls->host_outer.m;
  if (ls->n_outer > 0) {
    rc = upload_soa(ls->host_outer, ls->d_lines_outer, ls->Lo);
    if (rc) return rc;
  }
  { // direct index into the sorted centres (IcIndex)
    const int64_t m = H.m;
    const int x0 = m > 0 ? ls->ic.front() : 0, n_tab = m > 0 ? ls->ic.back() - x0 + 2 : 1;
    std::vector<int> first((size_t)n_tab);
    size_t q = 0;
    for (int t = 0; t < n_tab; ++t) {
      while (q < (size_t)m && ls->ic[q] < x0 + t) ++q;
      first[(size_t)t] = (int)q;
    }
    rc = ls->d_first.ensure(sizeof(int) * (size_t)n_tab);
    if (rc) return rc;
    HIPCHK(hipMemcpy(ls->d_first.p, first.data(), sizeof(int) * (size_t)n_tab, hipMemcpyHostToDevice));
    ls->first_x0 = x0;
    ls->first_n = n_tab;
  }
  if (!ls->work) { // a lineset of its own (level_set points its children at the parent's before the upload)
    ls->work = &ls->own_work;
    return ls->own_work.init();
  }
  return SR_OK;
}

extern "C" {

int sr_lineset_create(const sr_lines_desc *ld, const sr_isomolec_desc *iso, const sr_grid_desc *gd,
                      sr_lineset **out, int64_t *n_kept) {
  if (!ld || !iso || !gd || !out) return SR_ERR_ARG;
  *out = nullptr;
  if (ld->n_lines < 0 || iso->n_levels < 0 || !(gd->step > 0.0) || !(iso->mm > 0.0)) return SR_ERR_ARG;
  if (gd->n_grid < 2) return SR_ERR_ARG;
  if (gd->n_grid > 2000000) return SR_ERR_LIMIT;             // imxsig_long, spect_classes.py:29,362
  if (iso->n_levels > SR_MAX_LEVELS) return SR_ERR_LIMIT;
  if (ld->n_lines > 0 && (!ld->freq || !ld->a_coeff || !ld->e_lower || !ld->g_up || !ld->g_lo ||
                          !ld->air_broad || !ld->t_dep_broad))
    return SR_ERR_ARG;
  if (iso->n_levels > 0 && (!iso->level_energy || (ld->n_lines > 0 && (!ld->lev_up || !ld->lev_lo))))
    return SR_ERR_ARG;

  GridParams gp;
  gp.w0 = gd->w0;
  gp.gstep = gd->step;
  gp.n_grid = (int)gd->n_grid;
  // spect_classes.py:1446: np.arange(-imxsig*s/2, imxsig*s/2, s) = start + m*delta
  gp.lin_start = -(double)kImxsig * gp.gstep / 2;
  {
    const double lin_stop = (double)kImxsig * gp.gstep / 2;
    const double len = std::ceil((lin_stop - gp.lin_start) / gp.gstep);
    if (len != (double)kImxsig) {
      g_err = "np.arange window would not have 13010 points for this step (f2py would reject it)";
      return SR_ERR_UNSUPPORTED;
    }
    const double nxt = gp.lin_start + gp.gstep;
    gp.lin_delta = nxt - gp.lin_start;
  }

  const int nlev = iso->n_levels;
  const int64_t n = ld->n_lines;
  std::vector<int64_t> keep;
  keep.reserve(n);
  for (int64_t i = 0; i < n; ++i) {
    if (nlev > 0) {
      const int lu = ld->lev_up[i], ll = ld->lev_lo[i];
      // LinkToMolec must find both levels; its if/elif never finds the lower
      // level when it equals the upper one (spect_classes.py:135-150)
      if (lu < 0 || ll < 0 || lu >= nlev || ll >= nlev || lu == ll) continue;
    }
    keep.push_back(i);
  }
  const int64_t m = (int64_t)keep.size();
  std::vector<int> ic(m);
  std::vector<char> is_outer(m, 0);
  const int ng = gp.n_grid;
  for (int64_t q = 0; q < m; ++q) {
    const double f = ld->freq[keep[q]];
    if (!(f == f)) return SR_ERR_ARG;
    // closest_grid: first arg-min of |grid - f| (spect_classes.py:1941)
    double t = std::floor((f - gp.w0) / gp.gstep);
    long j0 = t < -4 ? -4 : (t > ng + 4 ? ng + 4 : (long)t);
    long a = std::max<long>(0, j0 - 2), b = std::min<long>(ng - 1, j0 + 3);
    if (a > b) { a = b = (j0 < 0 ? 0 : ng - 1); }
    long best = a;
    double bv = std::fabs(grid_at(gp, (int)a) - f);
    for (long j = a + 1; j <= b; ++j) {
      const double v = std::fabs(grid_at(gp, (int)j) - f);
      if (v < bv) { bv = v; best = j; }
    }
    ic[q] = (int)best;
    // A line farther than half a window (~3.25 cm-1) from the grid has its centre outside its own
    // window: humliv_bb takes an outer branch (lineshape.f:272, 358).  Kept apart, see launch_outer.
    WinX xf{gp.lin_start, gp.lin_delta, grid_at(gp, (int)best)};
    is_outer[q] = !(xf(1) < f && f < xf(kImxsig));
  }
  std::vector<int64_t> ord(m);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int64_t x, int64_t y) { return ic[x] < ic[y]; });

  sr_lineset *ls = new sr_lineset();
  ls->gp = gp;
  ls->mol = iso->mol;
  ls->iso = iso->iso;
  ls->mm = iso->mm;
  ls->n_levels = nlev;
  ls->e_lev.assign(iso->level_energy, iso->level_energy + nlev);

  // the line list in device layout, main and outer lines apart (both in centre order)
  HostLines all;
  all.m = m;
  all.md = (size_t)std::max<int64_t>(m, 1);
  all.d.assign(12 * all.md, 0.0);
  all.i.assign(3 * all.md, 0);
  const size_t md = all.md;
  const double h = kHcgs, c = kCcgs;
  std::vector<int64_t> sel_main, sel_outer;
  for (int64_t q = 0; q < m; ++q) {
    const int64_t s = keep[ord[q]];
    const double f = ld->freq[s];
    const double fact_2 = 2 * h * (c * c) * std::pow(f, 3.0); // spect_classes.py:1743
    const double b21 = ld->a_coeff[s] / fact_2;               // :1750
    const double b12 = ld->g_lo[s] != 0.0 ? b21 * ld->g_up[s] / ld->g_lo[s] : 0.0; // :1783
    const int lu = nlev > 0 ? ld->lev_up[s] : 0, ll = nlev > 0 ? ld->lev_lo[s] : 0;
    double *d = all.d.data();
    d[0 * md + q] = f;
    d[1 * md + q] = h * c * f;
    d[2 * md + q] = ld->a_coeff[s];
    d[3 * md + q] = b21;
    d[4 * md + q] = b12;
    d[5 * md + q] = ld->e_lower[s];
    d[6 * md + q] = ld->g_up[s];
    d[7 * md + q] = ld->g_lo[s];
    d[8 * md + q] = ld->air_broad[s];
    d[9 * md + q] = ld->t_dep_broad[s];
    d[10 * md + q] = nlev > 0 ? iso->level_energy[lu] : 0.0; // spect_classes.py:318-324
    d[11 * md + q] = nlev > 0 ? iso->level_energy[ll] : 0.0;
    all.i[0 * md + q] = ic[ord[q]];
    all.i[1 * md + q] = lu;
    all.i[2 * md + q] = ll;
    (is_outer[ord[q]] ? sel_outer : sel_main).push_back(q);
  }
  ls->host = subset(all, sel_main);
  ls->host_outer = subset(all, sel_outer);
  ls->n_in = n;
  std::vector<int> inpos((size_t)std::max<int64_t>(n, 1), -1);
  for (const int64_t q : sel_main) {
    inpos[(size_t)keep[ord[q]]] = (int)ls->in_main.size();
    ls->in_main.push_back(keep[ord[q]]);
  }
  for (const int64_t q : sel_outer) {
    inpos[(size_t)keep[ord[q]]] = -2 - (int)ls->in_outer.size();
    ls->in_outer.push_back(keep[ord[q]]);
  }
  int rc = lineset_upload(ls);
  if (!rc) rc = ls->d_inpos.ensure(sizeof(int) * inpos.size());
  if (!rc) {
    const hipError_t e = hipMemcpy(ls->d_inpos.p, inpos.data(), sizeof(int) * inpos.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy(inpos)");
  }
  if (rc) { sr_lineset_destroy(ls); return rc; }
  if (n_kept) *n_kept = m;
  *out = ls;
  return SR_OK;
}

int sr_lineset_set_bounds_temps(sr_lineset *ls, const double *temps_bounds, int n_layers) {
  if (!ls || n_layers < 0) return SR_ERR_ARG;
  if (!temps_bounds || n_layers == 0) {
    ls->bounds_temps.clear();
    return SR_OK;
  }
  for (int k = 0; k < n_layers; ++k)
    if (!(temps_bounds[k] > 0.0)) return SR_ERR_ARG;
  ls->bounds_temps.assign(temps_bounds, temps_bounds + n_layers);
  return SR_OK;
}

int sr_lineset_set_linear_weights(sr_lineset *ls, int on) {
  if (!ls) return SR_ERR_ARG;
  ls->linear_weights = on != 0;
  return SR_OK;
}

int sr_lineset_set_line_shape(sr_lineset *ls, const double *p_shift, const double *self_broad, int64_t n_lines) {
  if (!ls || ls->parent) return SR_ERR_ARG;
  if ((p_shift || self_broad) && n_lines != ls->n_in) return SR_ERR_ARG;
  for (int64_t i = 0; i < n_lines; ++i) {
    if (p_shift && !std::isfinite(p_shift[i])) return SR_ERR_ARG;
    if (self_broad && (!std::isfinite(self_broad[i]) || self_broad[i] < 0.0)) return SR_ERR_ARG;
  }
  // calls in flight on the handle and its sub-linesets read the arrays replaced below
  (void)hipDeviceSynchronize();
  // the per-level sub-linesets carry copies of the old data: dropped, cut again on their next use (level_set)
  for (std::vector<sr_lineset *> *sets : {&ls->level_sets, &ls->level_up_sets}) {
    for (sr_lineset *child : *sets) sr_lineset_destroy(child);
    sets->clear();
  }
  for (int which = 0; which < 2; ++which) {
    HostLines &H = which ? ls->host_outer : ls->host;
    const std::vector<int64_t> &in = which ? ls->in_outer : ls->in_main;
    H.p_shift.clear();
    H.self_broad.clear();
    if (p_shift) {
      H.p_shift.assign(H.md, 0.0);
      for (size_t p = 0; p < in.size(); ++p) H.p_shift[p] = p_shift[in[p]];
    }
    if (self_broad) {
      H.self_broad.assign(H.md, 0.0);
      for (size_t p = 0; p < in.size(); ++p) H.self_broad[p] = self_broad[in[p]];
    }
  }
  return lineset_upload(ls); // the arrays, and the bounds over the lines that depend on them (gamma_max, shift_max)
}

int sr_lineset_set_self_pressure(sr_lineset *ls, const double *p_self_hpa, int n_layers) {
  if (!ls || ls->parent || n_layers < 0) return SR_ERR_ARG;
  if (!p_self_hpa || n_layers == 0) {
    ls->self_press.clear();
    return SR_OK;
  }
  for (int k = 0; k < n_layers; ++k)
    if (!(p_self_hpa[k] >= 0.0) || !std::isfinite(p_self_hpa[k])) return SR_ERR_ARG;
  ls->self_press.assign(p_self_hpa, p_self_hpa + n_layers);
  return SR_OK;
}

int sr_lineset_destroy(sr_lineset *ls) {
  if (!ls) return SR_OK;
  (void)hipDeviceSynchronize(); // work of the last calls may still be in flight on the internal streams
  for (sr_lineset *child : ls->level_sets) sr_lineset_destroy(child);
  ls->level_sets.clear();
  for (sr_lineset *child : ls->level_up_sets) sr_lineset_destroy(child);
  ls->level_up_sets.clear();
  ls->d_lines_outer.release();
  ls->d_gscratch.release();
  ls->d_inpos.release();
  ls->d_sref.release();
  ls->s_str.release();
  ls->d_lines.release();
  ls->d_first.release();
  if (ls->work == &ls->own_work) ls->own_work.release();
  ls->mc.release();
  delete ls;
  return SR_OK;
}

} // extern "C"

// A table computed on the host and uploaded once per process and device (never freed): n doubles, written by fill
struct HostTableDev {
  std::mutex mu;
  std::map<int, double *> tabs;
  int get(size_t n, void (*fill)(double *), const double **out) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = tabs.find(dev);
    if (it == tabs.end()) {
      std::vector<double> h(n);
      fill(h.data());
      double *d = nullptr;
      HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), sizeof(double) * n));
      HIPCHK(hipMemcpy(d, h.data(), sizeof(double) * n, hipMemcpyHostToDevice));
      it = tabs.emplace(dev, d).first;
    }
    *out = it->second;
    return SR_OK;
  }
};
// Translation operator of the box-pair far field (0.8 MB)
static int m2l_table_dev(const double **out) {
  static HostTableDev t;
  return t.get((size_t)2 * kM2LOffsets * kM2LQ * kM2LRow, m2l_table_host, out);
}
// Downward-pass operator of the hierarchy (sr_l2l_kernel, 8 KB)
static int l2l_table_dev(const double **out) {
  static HostTableDev t;
  return t.get((size_t)2 * kFC * kFC, l2l_table_host, out);
}

// Per-layer scalars of a call (host, fp64): T, P [atm], 296/T, sqrt(2 N_A k T ln2 / MM), the same at the boundary
// temperatures, the level populations, Q(t_ref) / Q(T) and the vibrational ratios r_L of the strength weights (filled when
// q_ref > 0: the calls with HITRAN intensities), then three int rows: pole margin, source pole radius, widest zone.
//   mar: the lineset whose lines bound the margins -- the handle itself, or its PARENT for the far-only level passes of
//        the multi-channel route (every kernel of that route must place a (line, slot) pair on the same side of the
//        near / far split: the pole margin enters the admissibility threshold)
static size_t layer_stage_doubles(int nl, int npop) { return (size_t)nl * (10 + 2 * npop); }
// Grid points the centres of the lines of `mar` move by in a layer of p_atm, rounded up (sr_lineset_set_line_shape)
static int shift_points(const sr_lineset *mar, double p_atm, double gstep) {
  return mar->shift_max > 0.0 ? (int)std::ceil(std::min(mar->shift_max * p_atm / gstep, 1e6)) : 0;
}
static size_t layer_stage_bytes(int nl, int npop) { return sizeof(double) * layer_stage_doubles(nl, npop) + sizeof(int) * 3 * (size_t)nl; }
static int fill_layer_stage(const sr_lineset *ls, const sr_lineset *mar, const sr_lineset *bown, const sr_layers_desc *atm, double *T,
                            double q_ref = 0.0) {
  const int nl = atm->n_layers, nlev = ls->n_levels, npop = nlev > 0 ? nlev : 1;
  const size_t hl_doubles = layer_stage_doubles(nl, npop);
  const bool frozen = !bown->bounds_temps.empty();
  double *pa = T + nl, *tr = pa + nl, *sq = tr + nl, *ltr = sq + nl, *ltrb = ltr + nl, *sqb = ltrb + nl, *tb = sqb + nl,
         *pop = tb + nl, *qrat = pop + (size_t)nl * npop, *rvib = qrat + nl, *ps = rvib + (size_t)nl * npop;
  // sr_lineset_set_self_pressure (on the handle the caller holds, like the frozen boundaries): 0 when unset
  const bool self_p = !bown->self_press.empty() && (int)bown->self_press.size() == nl;
  std::vector<double> q(nl);
  if (atm->q_part) {
    std::copy(atm->q_part, atm->q_part + nl, q.begin());
  } else {
    const int rc = sr_calc_partition_sum(ls->mol, ls->iso, atm->temps, nl, q.data());
    if (rc) return rc;
  }
  for (int k = 0; k < nl; ++k) {
    T[k] = atm->temps[k];
    pa[k] = atm->press[k] * kHpaToAtm;                                        // spect_classes.py:2034
    tr[k] = kTref / T[k];                                                     // :1972
    sq[k] = std::sqrt(2 * kAvogadro * kKcgs * T[k] * kLn2 / ls->mm);          // :1984
    ltr[k] = std::log(tr[k]);
    ps[k] = self_p ? bown->self_press[k] * kHpaToAtm : 0.0;
    {
      const double Tb = frozen ? bown->bounds_temps[k] : T[k]; // where the region boundaries are placed
      tb[k] = Tb;
      ltrb[k] = std::log(kTref / Tb);
      sqb[k] = std::sqrt(2 * kAvogadro * kKcgs * Tb * kLn2 / ls->mm);
    }
    {
      // pole margin of the far-field expansions: the region-1 rational has its poles at
      // |x| = sqrt(1/2 + ry^2), i.e. within 0.71 dw' of the line centre on the real axis.
      // Frozen boundaries (sr_lineset_set_bounds_temps): the zone of a line is placed with the widths of the
      // boundary temperature Tb, the poles sit where the call's own widths put them -- the bounds below cover both
      // (with the call's T alone a frozen zone wider than zmax, Tb > T, lost its outer points: ADVICE round 3).
      const double sq_w = std::max(sq[k], sqb[k]);
      const double dwp_max = mar->freq_max / kCcgs * sq_w / std::sqrt(kLn2);
      int *pmh = reinterpret_cast<int *>(T + hl_doubles);
      // Pressure shift (sr_lineset_set_line_shape).  The three bounds below are distances in grid points from a line's
      // window centre ic -- what every candidate range and ownership test of the kernels is written in -- and each
      // assumed the centre within half a cell of grid[ic].  The shifted centre x0' = Freq + p_shift P lies within
      // 1/2 + |p_shift| P / step <= 1/2 + sk of it, so each grows by sk (0 without shifts):
      //   pole margin: the poles sit within 0.71 dw' of x0', i.e. within 0.71 dw' / step + 1/2 + sk of ic; a box
      //     admissible at kTheta h + pm from ic is then still kTheta h from the nearest pole, which is what the
      //     truncation bound is written for (sr_kernels.hpp, ff_thr2);
      //   source pole radius: the multipole series of a source box converges outside the largest distance of a pole
      //     of its lines from the box centre, h + 1/2 + sk + |pole| (m2l_separated compares h + pm_src);
      //   widest zone: region 1 starts (lw + 15 dw') / step from x0', i.e. that + 1/2 + sk from ic.
      const int sk = shift_points(mar, pa[k], ls->gp.gstep);
      pmh[k] = (int)std::ceil(0.71 * dwp_max / ls->gp.gstep) + 1 + sk;
      // box-pair mode: the multipole series of a source box converges outside the largest |pole| =
      // sqrt(1/2 + ry^2) dw' = sqrt(dw'^2 / 2 + lw^2) of its lines (bound over the lines of the layer)
      const double trb = frozen ? kTref / bown->bounds_temps[k] : tr[k];
      const double lw_max = mar->gamma_max * pa[k] *
                            std::max(std::max(std::pow(tr[k], mar->ndep_min), std::pow(tr[k], mar->ndep_max)),
                                     std::max(std::pow(trb, mar->ndep_min), std::pow(trb, mar->ndep_max)));
      const double pole = std::sqrt(0.5 * dwp_max * dwp_max + lw_max * lw_max) / ls->gp.gstep;
      pmh[nl + k] = (int)std::ceil(std::min(pole, 1e6)) + sk;
      // widest region-2/3/4 zone of the layer, in grid points from the line centre: region 1 starts where
      // |x| - ry >= 15 (lineshape.f:447-454), i.e. (lw + 15 dw') / step points out, +-1 for the nint and the
      // centre's offset inside its grid cell.  A bound over the lines (every kernel reads this one value, so they
      // agree on who evaluates what); kernels clamp it to the window half-width.
      pmh[2 * nl + k] = (int)std::min(std::ceil((lw_max + 15.0 * dwp_max) / ls->gp.gstep) + 2.0 + sk, (double)kHalf);
    }
    if (nlev > 0) {
      for (int lv = 0; lv < nlev; ++lv) {
        const double vibt = atm->tvib ? atm->tvib[(size_t)lv * nl + k] : T[k]; // smm:2062-2065
        pop[(size_t)k * npop + lv] = std::exp(-kC2 * ls->e_lev[lv] / vibt) / q[k]; // smm:2073
      }
    } else {
      pop[k] = 1 / q[k]; // smm:2054
    }
    if (q_ref > 0.0) { // the strength weights: Q(t_ref) / Q(T), vibtemp_to_ratio(E_L, Tvib_L, T) (1 for the 'all' set)
      qrat[k] = q_ref / q[k];
      for (int lv = 0; lv < npop; ++lv) {
        const double e = nlev > 0 ? ls->e_lev[lv] : 0.0, vibt = (nlev > 0 && atm->tvib) ? atm->tvib[(size_t)lv * nl + k] : T[k];
        rvib[(size_t)k * npop + lv] = std::exp(-kC2 * e / vibt) / std::exp(-kC2 * e / T[k]);
      }
    }
  }
  return SR_OK;
}
// The device view of a pushed layer stage: the scalars, and the three int rows behind them by name
struct LayerStage {
  LayersDev A;
  const int *pm, *pm_src, *zmax; // [n_layers] each: pole margin | source pole radius | widest zone (host bounds, see fill_layer_stage)
};
// A call's layer stage through slot S: prepare, fill (host, fp64), push on `st`.  wait_for: an event `st` waits for
// between the fill and the copy (what last read the slot's device mirror), or nullptr.  boundaries = false: the call
// places no region boundaries (sr_line_strengths_dev), so frozen ones do not apply.
static int stage_layers(Stager &S, const sr_lineset *ls, const sr_lineset *mar, const sr_lineset *bown, const sr_layers_desc *atm,
                        double q_ref, bool boundaries, hipEvent_t wait_for, hipStream_t st, LayerStage *out) {
  const int nl = atm->n_layers, npop = ls->n_levels > 0 ? ls->n_levels : 1;
  const size_t bytes = layer_stage_bytes(nl, npop);
  int rc = S.prepare(bytes);
  if (rc) return rc;
  rc = fill_layer_stage(ls, mar, bown, atm, S.host<double>(), q_ref);
  if (rc) return rc;
  if (wait_for) HIPCHK(hipStreamWaitEvent(st, wait_for, 0));
  rc = S.push(bytes, st);
  if (rc) return rc;
  const bool frozen = boundaries && !bown->bounds_temps.empty(); // sr_lineset_set_bounds_temps
  const double *dl = S.d.as<double>();
  LayersDev &A = out->A;
  A.temps = dl; A.p_atm = dl + nl; A.trat = dl + 2 * nl; A.sqk = dl + 3 * nl; A.ltrat = dl + 4 * nl;
  A.ltrat_b = dl + 5 * nl; A.sqk_b = dl + 6 * nl; A.temps_b = dl + 7 * nl; A.pop = dl + 8 * nl;
  A.qrat = A.pop + (size_t)nl * npop; A.rvib = A.qrat + nl; A.ps_atm = A.rvib + (size_t)nl * npop;
  A.frozen = frozen ? 1 : 0;
  A.linear_w = frozen && bown->linear_weights ? 1 : 0;
  A.n_layers = nl; A.n_pop = npop;
  A.sqrt_ln2 = std::sqrt(kLn2);            // spect_classes.py:1999
  A.sqrt_pi_ln2 = std::sqrt(kPi / kLn2);   // :1997
  out->pm = reinterpret_cast<const int *>(dl + layer_stage_doubles(nl, npop));
  out->pm_src = out->pm + nl;
  out->zmax = out->pm + 2 * nl;
  return SR_OK;
}
// The far-field box hierarchy of a shard of n_pts points (the part of FarParams every kernel agrees on)
static void far_hierarchy(size_t n_pts, int nl, FarParams *fp) {
  fp->n_levels = kMaxFarLevels;
  fp->n_layers = nl;
  fp->n_boxes_total = 0;
  fp->top_first = n_pts <= 16384 ? 1 : 0; // see sr_farfield_kernel
  fp->folded0 = 0;
  for (int lv = 0; lv < kMaxFarLevels; ++lv) {
    const int W = 64 << lv;
    fp->box_count[lv] = (int)((n_pts + W - 1) / W);
    fp->box_off[lv] = fp->n_boxes_total;
    fp->n_boxes_total += fp->box_count[lv];
  }
}
// The FarParams of a pass.  kind: per-line expansions at every level, the same by the sparse sets' own kernel
// (sr_farfield_rows_kernel: a box for eight layers per wave), or box pairs with the layout of their source boxes
// (*n_src_total of them per layer: the caller sets mom and tab).  folded0 = 0 and no lines beyond the grid ends:
// coef_op sets those for its own passes.
enum FarKind { kFarPerLine, kFarPerLineRows, kFarBoxPairs };
static FarParams far_params(size_t n_pts, const LayerStage &S, FarKind kind, double *coef, int *n_src_total = nullptr) {
  FarParams fp;
  far_hierarchy(n_pts, S.A.n_layers, &fp);
  fp.pm = S.pm; fp.pm_src = S.pm_src; fp.coef = coef;
  fp.m2l = kind == kFarBoxPairs ? 1 : 0;
  fp.rows = kind == kFarPerLineRows ? 1 : 0;
  fp.disp_lo_end = fp.disp_hi_begin = 0;
  fp.mom = nullptr; fp.tab = nullptr;
  // level-0 source boxes: kSrcPad left of the shard, the shard, the window half-width right of it; a whole
  // number of widest boxes, so that every level halves exactly
  const int top_boxes = fp.m2l ? (int)(((size_t)kSrcPad * 64 + n_pts + kHalf + 64) >> (6 + kMaxFarLevels - 1)) + 1 : 0;
  int total = 0;
  for (int lv = 0; lv < kMaxFarLevels; ++lv) {
    fp.n_src[lv] = top_boxes << (kMaxFarLevels - 1 - lv);
    fp.src_off[lv] = total;
    total += fp.n_src[lv];
  }
  if (n_src_total) *n_src_total = total;
  return fp;
}
// Sparse line sets (the per-level sub-linesets of the pair tables: 9-15 % of a hot-band list): the box-pair far field
// has a fixed cost per box and layer -- S2M, M2M, M2L over every box whatever it holds -- that the per-line
// expansions at every level (mode 1) do not have: below ~0.37 lines per grid point they are the faster route
// (tools/ff_mode_crossover.py: 0.3: 2.54 vs 2.61 ms, 0.4: 3.07 vs 3.03, 1.0: 6.74 vs 5.62; the 12 pair tables of the
// configs[1] list 19.1 vs 21.5 ms).  Mode 3 (the default) switches at 0.35.
static bool is_sparse_set(const sr_lineset *ls, int far_mode) {
  constexpr double sparse_thr = 0.35;
  return far_mode == 3 && (double)ls->n_lines < sparse_thr * (double)ls->gp.n_grid;
}
// The lines whose window [ic-6505, ic+6504] meets the shard [g_lo, g_hi): line_lo / n_sub of the lineset's centre index
static IcIndex shard_lines(const sr_lineset *ls, int64_t g_lo, int64_t g_hi) {
  const auto lo_it = std::lower_bound(ls->ic.begin(), ls->ic.end(), (int)g_lo - (kHalf - 1));
  const auto hi_it = std::upper_bound(ls->ic.begin(), ls->ic.end(), (int)g_hi - 1 + kHalf);
  return IcIndex{ls->d_first.as<int>(), ls->first_x0, ls->first_n, (int)(lo_it - ls->ic.begin()), (int)(hi_it - lo_it)};
}

// The argument checks of a coefficient call: handle, layers, shard and the (T, P) of every layer.  entry_only: what
// the entry points of the level tables need before they size their scratch -- the rest is answered by coef_op /
// mc_pass below them, which check in full.
static int check_coef_call(const sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, bool entry_only = false) {
  if (!ls || !atm || atm->n_layers <= 0 || g_lo < 0 || g_lo >= g_hi) return SR_ERR_ARG;
  if (entry_only) return SR_OK;
  if (!atm->temps || !atm->press || g_hi > ls->gp.n_grid) return SR_ERR_ARG;
  for (int k = 0; k < atm->n_layers; ++k)
    if (!(atm->temps[k] > 0.0) || !(atm->press[k] >= 0.0)) return SR_ERR_ARG;
  return SR_OK;
}

// What a coefficient call on a handle with sr_lineset_set_line_shape / sr_lineset_set_self_pressure data must hold
// (include/spectrobot_hip.h), on the host, before anything is copied or launched.  root: the handle the caller holds
// (a sub-lineset's parent).  Nothing to check, and SR_OK, for a handle without the data.
static int check_line_shape(const sr_lineset *root, const sr_layers_desc *atm) {
  const int nl = atm->n_layers;
  if (!atm->press || !atm->temps) return SR_OK; // (refused by check_coef_call)
  if (!root->self_press.empty()) {
    if ((int)root->self_press.size() != nl) {
      g_err = "sr_lineset_set_self_pressure was given another number of layers than this call";
      return SR_ERR_ARG;
    }
    for (int k = 0; k < nl; ++k)
      if (!(root->self_press[k] <= atm->press[k])) {
        g_err = "sr_lineset_set_self_pressure: p_self above the layer's pressure";
        return SR_ERR_ARG;
      }
  }
  if (!(root->shift_max > 0.0)) return SR_OK;
  const GridParams &gp = root->gp;
  for (int k = 0; k < nl; ++k)
    if (root->shift_max * (atm->press[k] * kHpaToAtm) > (double)SR_MAX_SHIFT_POINTS * gp.gstep) {
      g_err = "pressure shift beyond SR_MAX_SHIFT_POINTS grid steps";
      return SR_ERR_LIMIT;
    }
  // humliv_bb's branch must stay the one the line was sorted into: the outer lines, and the main lines centred beyond
  // a grid end (the only ones whose centre is not within half a step of their window centre) -- few of either
  auto inside = [&](const HostLines &H, int64_t q, double p_atm) {
    const WinX xf{gp.lin_start, gp.lin_delta, grid_at(gp, H.i[q])};
    const double x0 = H.d[q] + H.p_shift[q] * p_atm;
    return xf(1) < x0 && x0 < xf(kImxsig);
  };
  const HostLines &Ho = root->host_outer, &Hm = root->host;
  for (int k = 0; k < nl; ++k) {
    const double p_atm = atm->press[k] * kHpaToAtm;
    for (int64_t q = 0; q < Ho.m && !Ho.p_shift.empty(); ++q)
      if (inside(Ho, q, p_atm)) {
        g_err = "pressure shift moves an outer line's centre into its own window";
        return SR_ERR_UNSUPPORTED;
      }
    for (int64_t q = 0; q < Hm.m; ++q) {
      if (q == root->n_disp_lo) q = std::max(q, Hm.m - root->n_disp_hi);
      if (q >= Hm.m) break;
      if (!inside(Hm, q, p_atm)) {
        g_err = "pressure shift moves a line's centre out of its own window";
        return SR_ERR_UNSUPPORTED;
      }
    }
  }
  return SR_OK;
}

// The layers of a call in batches of at most `batch`: fn(sub, k0) for every [k0, k0 + sub.n_layers), with the batch's
// slice of temps / press / q_part and of the vibrational temperatures (keep_tvib; else none: no populations enter the
// level spectra), and with bown->bounds_temps (sr_lineset_set_bounds_temps) cut to the batch, restored on every way out.
template <class Fn>
static int for_layer_batches(const sr_layers_desc *atm, sr_lineset *bown, int nlev, bool keep_tvib, int batch, Fn fn) {
  const int nl = atm->n_layers;
  if (!bown->bounds_temps.empty() && (int)bown->bounds_temps.size() != nl) {
    g_err = "sr_lineset_set_bounds_temps was given another number of layers than this call";
    return SR_ERR_ARG;
  }
  sr_layers_desc sub = *atm;
  if (!keep_tvib) sub.tvib = nullptr;
  if (batch >= nl) return fn(sub, 0);
  const std::vector<double> bounds_all = bown->bounds_temps, self_all = bown->self_press;
  struct Restore {
    sr_lineset *ls; const std::vector<double> &all, &self;
    ~Restore() { ls->bounds_temps = all; ls->self_press = self; }
  } restore{bown, bounds_all, self_all};
  std::vector<double> tv;
  for (int k0 = 0; k0 < nl; k0 += batch) {
    const int n = sub.n_layers = std::min(batch, nl - k0);
    sub.temps = atm->temps + k0;
    sub.press = atm->press + k0;
    sub.q_part = atm->q_part ? atm->q_part + k0 : nullptr;
    if (keep_tvib && atm->tvib) { // [n_levels][n_layers] -> the batch's columns
      tv.resize((size_t)nlev * n);
      for (int lv = 0; lv < nlev; ++lv)
        std::copy(atm->tvib + (size_t)lv * nl + k0, atm->tvib + (size_t)lv * nl + k0 + n, tv.begin() + (size_t)lv * n);
      sub.tvib = tv.data();
    }
    if (!bounds_all.empty()) bown->bounds_temps.assign(bounds_all.begin() + k0, bounds_all.begin() + k0 + n);
    if (!self_all.empty()) bown->self_press.assign(self_all.begin() + k0, self_all.begin() + k0 + n);
    const int rc = fn(sub, k0);
    if (rc) return rc;
  }
  return SR_OK;
}

// Bytes per layer of a coefficient op.  The per-(line, layer) record tables cost 128 B each, the far-field scratch of a
// layer (local coefficients of all levels' target boxes, multipole moments of the source boxes) 1 KB per 64 grid points
// + 1.3 KB per 64 points of grid and window halo; a long LOS (the reference allows imxstp = 8000 steps) is processed
// in layer batches that keep them under g_table_budget.
static size_t coef_bytes_per_layer(const sr_lineset *ls, size_t n_pts, int far_field, int overlap) {
  const size_t far_per_layer = !far_field ? 0
      : (2 * (n_pts / 64 + 2)) * (size_t)(2 * kFC) * sizeof(double) +
        (far_field == 2 ? (2 * ((n_pts + 64 * kSrcPad + kHalf) / 64 + 16)) * (size_t)kMomPerBox * sizeof(double) : 0);
  return (size_t)std::max<int64_t>(ls->n_lines, 1) * (sizeof(FastRec) + sizeof(ColdRec)) * (overlap ? 2 : 1) + far_per_layer // two table sets with overlap
         + (overlap ? 2 * sizeof(double) * n_pts : 0)           // the zones kernel's private sums (small shards)
         + sizeof(OuterRec) * (size_t)std::max(ls->n_outer, 0); // records of the outer lines
}
// Bytes per row of a multi-channel pass: the full list's records + every far pass's coefficients (coef_row doubles per
// pass and row) + what the largest level pass needs of the shared CoefWork (two table sets, far-field scratch)
static size_t mc_bytes_per_row(const sr_lineset *ls, size_t n_pts, size_t coef_row, int n_far) {
  return (size_t)std::max<int64_t>(ls->n_lines, 1) * (sizeof(FastRec) + sizeof(ColdRec)) * 4 +
         sizeof(double) * coef_row * (size_t)(n_far + 2) + 4 * ((n_pts + 64 * kSrcPad + kHalf) / 64 + 16) * (size_t)kMomPerBox * sizeof(double);
}

// Options of coef_op beyond the public entry points'.
//   far_coef: a FAR-ONLY pass for the multi-channel route (mc_pass) -- tables and the far-field chain only, the
//   coefficients [n_layers][n_boxes_total][2][kFC] written there and folded down to level 0 (sr_l2l_kernel: wider levels
//   hold partial sums afterwards, level 0 everything); no near kernels, no outer lines, abs_out / emi_out
//   untouched (may be null); the margins are the PARENT's (fill_layer_stage); *far_has = whether any line met the shard.
//   q_ref: Q(t_ref) of the HITRAN intensities, for the strength weights (kWeightStrength); 0 otherwise.
struct CoefOpt {
  double *far_coef = nullptr;
  bool *far_has = nullptr;
  double q_ref = 0.0;
};
// One snapshot of the mode switches per call (coef_op), shared by its layer batches
struct CoefModes {
  int variant, far_field; // far_field: 0 exact, 1 per-line expansions, 2 box pairs (mode 3 resolved: is_sparse_set)
  bool timing, sparse_set, counting;
  // 1: the decoupled, phased pipeline (far-field modes); 0: the kernels one after the other on the caller's stream, on
  // table set 0 -- sr_set_overlap(0), the exact mode and the counting passes (whose counters are zeroed and read on the
  // caller's stream).  (Round 3's order, overlap 2, was the A/B partner of rounds 4-5 and is gone.)
  int overlap;
  int reps[6]; // launches of each kernel (measurement hook, serial schedule only: see g_repeat_kernel)
};
// What the kernels of one far-field call share, whichever schedule issues them
struct CoefKernels {
  CoefWork &w;
  int b; // table set
  ShardTables t;
  FarParams fp;
  const GridParams &gp;
  bool far_only, timing;
  double *abs_out, *emi_out;
  unsigned long long *cnt;
  hipStream_t st;  // the caller's stream
  const int *reps; // CoefModes::reps
};

// The far-field chain on stream fs: per-line expansions (all levels, or level 0 of the box-pair mode), then the box
// pairs -- moments + upward pass, translations --, then the downward pass behind them.  s2m_done: an event to record
// behind S2M + M2M, or nullptr.
static int far_chain(const CoefKernels &k, hipStream_t fs, hipEvent_t s2m_done = nullptr) {
  for (int r = 0; r < k.reps[1]; ++r) LAUNCHCHK(launch_farfield(k.t, k.fp, k.cnt, fs));
  if (k.fp.m2l) {
    for (int r = 0; r < k.reps[2]; ++r) LAUNCHCHK(launch_m2l(k.t, k.fp, k.cnt, fs, 1));
    if (s2m_done) HIPCHK(hipEventRecord(s2m_done, fs));
    for (int r = 0; r < k.reps[3]; ++r) LAUNCHCHK(launch_m2l(k.t, k.fp, k.cnt, fs, 2));
  }
  if (k.far_only || k.fp.folded0) { // the downward pass: the wider levels into the level-0 coefficients
    const double *l2l_tab = nullptr;
    const int rc = l2l_table_dev(&l2l_tab);
    if (rc) return rc;
    LAUNCHCHK(launch_l2l(k.fp.coef, k.t.n_layers, k.fp, l2l_tab, fs));
  }
  return SR_OK;
}

// The serial schedule: chain, wings, zones one after the other on the caller's stream
static int coef_serial(const CoefKernels &k) {
  CoefWork &w = k.w;
  w.overlapped = false;
  const int rc = far_chain(k, k.st); // (the downward pass's time falls into the far-field group's slot)
  if (rc) return rc;
  if (k.timing) HIPCHK(hipEventRecord(w.ev[2], k.st));
  // wings (writes) then zones (adds); the repeat hook's zones launches store instead (idempotent)
  for (int part = 1; part <= 2 && !k.far_only; ++part) {
    const int n_rep = k.reps[part == 1 ? 5 : 4];
    for (int r = 0; r < n_rep; ++r)
      LAUNCHCHK(launch_near(part, part == 2 && n_rep == 1, k.t, k.gp, k.fp, k.abs_out, k.emi_out, k.cnt, k.st));
    if (k.timing) HIPCHK(hipEventRecord(w.ev[2 + part], k.st));
  }
  return SR_OK;
}

// The decoupled, phased pipeline (round 4).  Between consecutive calls only the caller-visible output orders things:
// the zones kernel (tables -> private sums), the far-field chain (tables -> coefficients) and the preparation of
// the tables touch scratch of the call's own parity and nothing of the caller's, so they run on internal streams,
// beside the previous call's kernels; only the wings kernel (zones' sums + near region 1 + polynomials -> abs / emi)
// sits on the caller's stream.  Who runs beside whom is decided by what FITS beside whom
// (profiles/r04_timeline_*.txt, tools/kernel_resources.sh): 16 zones waves fill a CU -- 120 VGPRs each, 4 x 120 of a
// SIMD's 512, and 16 x 10 KB = all of its LDS -- and a retiring zones wave frees exactly one such slot, which the
// next zones wave takes unless the other kernel's wave fits it: the wings kernel (80 VGPRs), M2M / M2L (106 / 104)
// and the one-wave blocks of the preparation (104 VGPRs, 5 KB) do, the level-0 pass (140) and S2M (154) do not and
// starved beside the zones kernel until it drained -- then S2M -> M2M -> M2L ran alone, latency-bound, for 0.66 ms
// of every 5.6 ms step (round 3: the zones kernel forked off the caller's stream, the chain on it; the four-wave
// blocks of the preparation, 20 KB of LDS each, ran only when everything else had drained).  So the step has two
// phases: B = [wings(c) | level-0 pass(c + 1) | S2M(c + 1)] -- short waves that share the chip fairly --, then
// A = [zones(c + 1) | M2M, M2L(c + 1) | prep(c + 2)]; the zones kernel is GATED behind the level-0 pass and S2M of
// its own call (it needs neither), which is what keeps it from flooding the chip before they are through.
// These phases come out of TWO internal streams whose own order is the phase order -- not a stream per part, ordered
// by events on what each reads alone: that was the layout until profiles/two_stream_pipeline_ab.txt, and its overlap
// held only where each of the five streams had a hardware queue of its own, not on the runtime's default of four:
//   far_st:  prep(c) -> level-0(c) -> S2M, M2M(c) -> M2L(c) -> prep(c + 1) -> ..   near_st: zones(c)
// M2L(c + 1) and prep(c + 2) follow S2M(c + 1) on far_st and so run beside zones(c + 1), which that S2M releases;
// the level-0 pass and S2M of a call run one after the other, both beside wings(c).  Every wait below is on an event
// recorded earlier in host order, so no two streams can wait for each other.
static int coef_decoupled(const CoefKernels &k, hipStream_t far_st, hipStream_t near_st) {
  CoefWork &w = k.w;
  const int b = k.b;
  const size_t n_out = (size_t)(k.t.g_hi - k.t.g_lo) * k.t.n_layers;
  double *z_abs = nullptr, *z_emi = nullptr;
  if (!k.far_only) {
    const int rc = w.d_zone2[b].ensure(sizeof(double) * 2 * n_out);
    if (rc) return rc;
    z_abs = w.d_zone2[b].as<double>();
    z_emi = z_abs + n_out;
  }
  // (the buffers of parity b were last read by the wings kernel two calls ago: the preparation waited for that)
  // far-field chain, behind the table preparation on its stream: level-0 pass, moments + upward pass, translations, downward pass
  const int rc = far_chain(k, far_st, w.ev_s2m_done[b]);
  if (rc) return rc;
  HIPCHK(hipEventRecord(w.ev_far_done[b], far_st));
  if (k.far_only) { // the coefficients are the result: the caller's stream sees them complete
    HIPCHK(hipStreamWaitEvent(k.st, w.ev_far_done[b], 0));
  } else {
    // zones: needs the tables only; gated behind the kernels that cannot run beside it: S2M (on far_st the tables and
    // the level-0 pass precede it), or, without box pairs, the level-0 pass, which is then the whole chain
    HIPCHK(hipStreamWaitEvent(near_st, k.fp.m2l ? w.ev_s2m_done[b] : w.ev_far_done[b], 0));
    LAUNCHCHK(launch_near(2, 0, k.t, k.gp, k.fp, z_abs, z_emi, k.cnt, near_st));
    HIPCHK(hipEventRecord(w.ev_zones_done[b], near_st));
    HIPCHK(hipStreamWaitEvent(k.st, w.ev_far_done[b], 0));
    if (k.timing) HIPCHK(hipEventRecord(w.ev[2], k.st));
    HIPCHK(hipStreamWaitEvent(k.st, w.ev_zones_done[b], 0));
    LAUNCHCHK(launch_near(1, 0, k.t, k.gp, k.fp, k.abs_out, k.emi_out, k.cnt, k.st, z_abs, z_emi));
  }
  if (k.timing) HIPCHK(hipEventRecord(w.ev[3], k.st));
  if (k.timing) HIPCHK(hipEventRecord(w.ev[4], k.st));
  w.overlapped = true;
  return SR_OK;
}

// One layer batch of coef_op: stage the layers, select the lines, tables, far chain and near kernels in one of the two
// schedules (or the exact kernels), outer lines, end of call
static int coef_batch(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *abs_out, double *emi_out,
                      hipStream_t st, const WeightMode W, const CoefOpt &opt, const CoefModes &m) {
  const bool far_only = opt.far_coef != nullptr;
  CoefWork &w = *ls->work;
  // frozen region boundaries are set on the handle the caller holds: a per-level sub-lineset follows its parent's
  const sr_lineset *const bown = ls->parent ? ls->parent : ls;
  const int nl = atm->n_layers, overlap = m.overlap;
  const size_t n_pts = (size_t)(g_hi - g_lo);
  // Table set of this call and the stream its preparation runs on.  With overlap, call c + 1
  // prepares set (c + 1) % 2 on far_st while the kernels of call c (which the caller's stream is
  // still running) read set c % 2: the HBM-write-bound prep kernel hides behind the VALU-bound ones.
  const int b = overlap ? (w.parity ^= 1) : 0;
  hipStream_t pst = st;
  // Order this call after the previous one on this handle (see ev_last_done): a no-op when both use
  // the same stream.  The next call's table preparation (pst) needs only its own table set to be free.
  if (w.last_done_recorded) HIPCHK(hipStreamWaitEvent(st, w.ev_last_done, 0));
  hipStream_t far_st = nullptr, near_st = nullptr; // the pipeline's two streams (see CoefWork)
  if (overlap) {
    int rcs = w.pipeline_streams(&far_st, &near_st);
    if (!rcs) rcs = w.pipeline_events();
    if (rcs) return rcs;
    pst = far_st;
  }
  // per-layer scalars; set b was last read by the kernels of the call before the previous one
  LayerStage S;
  int rc = stage_layers(w.s_layers[b], ls, far_only && ls->parent ? ls->parent : ls, bown, atm, opt.q_ref, true,
                        overlap && w.free_recorded[b] ? w.ev_tables_free[b] : nullptr, pst, &S);
  if (rc) return rc;
  const IcIndex ix = shard_lines(ls, g_lo, g_hi);
  const int line_lo = ix.line_lo, n_sub = ix.n_sub;
  w.timed = w.overlapped = w.counted = false;
  unsigned long long *d_cnt = nullptr;
  if (m.counting) {
    rc = w.d_counts.ensure(sizeof(unsigned long long) * kCntN);
    if (rc) return rc;
    d_cnt = w.d_counts.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * kCntN, st));
  }
  // lines with their centre outside their own window: added after the main kernels (launch_outer)
  auto add_outer = [&]() -> int {
    if (ls->n_outer <= 0) return SR_OK;
    int rc2 = w.d_outer_recs.ensure(sizeof(OuterRec) * (size_t)ls->n_outer * nl);
    if (rc2) return rc2;
    LAUNCHCHK(launch_outer(ls->Lo, ls->n_outer, S.A, ls->gp, W, w.d_outer_recs.as<OuterRec>(), (int)g_lo, (int)g_hi,
                           abs_out, emi_out, st));
    return SR_OK;
  };
  if (opt.far_has) *opt.far_has = n_sub > 0;
  if (n_sub <= 0 && far_only) return SR_OK; // nothing staged on the internal streams: no event to record
  if (n_sub <= 0) {
    HIPCHK(hipMemsetAsync(abs_out, 0, sizeof(double) * n_pts * nl, st));
    HIPCHK(hipMemsetAsync(emi_out, 0, sizeof(double) * n_pts * nl, st));
    if (ls->n_outer <= 0) return SR_OK;
    // the layer scalars were pushed on pst: the caller's stream must see them
    if (overlap) {
      HIPCHK(hipEventRecord(w.ev_prep_done[b], pst));
      HIPCHK(hipStreamWaitEvent(st, w.ev_prep_done[b], 0));
    }
    rc = add_outer();
    if (rc) return rc;
    return w.end_call(st, overlap ? b : -1);
  }
  DevBuf &d_fast = w.d_fast[b], &d_cold = w.d_cold[b];
  rc = d_fast.ensure(sizeof(FastRec) * ((size_t)n_sub * nl + 1));
  if (!rc) rc = d_cold.ensure(sizeof(ColdRec) * ((size_t)n_sub * nl + 1));
  if (rc) return rc;
  const ShardTables t{d_fast.as<FastRec>(), d_cold.as<ColdRec>(), ix, S.zmax, nl, (int)g_lo, (int)g_hi};
  if (m.timing) HIPCHK(hipEventRecord(w.ev[0], pst));
  // cold records: far-field mode reads them for zones inside the shard only, exact mode for window ends too
  for (int r = 0; r < m.reps[0]; ++r)
    LAUNCHCHK(launch_prep(ls->L, S.A, ls->gp, W, line_lo, n_sub, far_only ? INT_MAX / 2 : (m.far_field ? (int)g_lo : INT_MIN / 2),
                          far_only ? INT_MIN / 2 : (m.far_field ? (int)g_hi - 1 : INT_MAX / 2), d_fast.as<FastRec>(),
                          d_cold.as<ColdRec>(), pst)); // (far-only: an empty cold range, no region-2..4 records)
  if (m.timing) HIPCHK(hipEventRecord(w.ev[1], pst));
  if (overlap) { // the caller's stream takes over once the tables are ready
    HIPCHK(hipEventRecord(w.ev_prep_done[b], pst));
    HIPCHK(hipStreamWaitEvent(st, w.ev_prep_done[b], 0));
    if (m.timing) HIPCHK(hipEventRecord(w.ev_op0, st));
  }
  if (m.far_field) {
    int n_src = 0;
    const FarKind kind = m.far_field == 2 ? kFarBoxPairs : m.sparse_set ? kFarPerLineRows : kFarPerLine;
    CoefKernels k{w, b, t, far_params(n_pts, S, kind, opt.far_coef, &n_src), ls->gp, far_only, m.timing, abs_out, emi_out, d_cnt, st, m.reps};
    FarParams &fp = k.fp;
    if (fp.m2l) {
      rc = w.d_mom[b].ensure(sizeof(double) * (size_t)n_src * nl * kMomPerBox);
      if (rc) return rc;
      fp.mom = w.d_mom[b].as<double>();
      rc = m2l_table_dev(&fp.tab);
      if (rc) return rc;
    }
    if (!far_only) {
      rc = w.d_coef[b].ensure(sizeof(double) * (size_t)nl * fp.n_boxes_total * 2 * kFC);
      if (rc) return rc;
      fp.coef = w.d_coef[b].as<double>();
    }
    // box-pair mode: the downward pass folds every level into level 0 behind M2L (both schedules) and the near-wings
    // kernel evaluates ONE polynomial per point; the per-line mode of sparse sets keeps a polynomial per level
    fp.folded0 = fp.m2l && !far_only ? 1 : 0;
    fp.disp_lo_end = (int)std::min<int64_t>(std::max<int64_t>(ls->n_disp_lo - line_lo, 0), n_sub);
    fp.disp_hi_begin = (int)std::min<int64_t>(std::max<int64_t>(ls->n_lines - ls->n_disp_hi - line_lo, 0), n_sub);
    rc = overlap ? coef_decoupled(k, far_st, near_st) : coef_serial(k);
    if (rc) return rc;
    w.n_timed = 4;
  } else {
    w.n_timed = 3;
    for (int which = 0; which < 2; ++which) {
      LAUNCHCHK(launch_abscoeff(m.variant, which, t, ls->gp, abs_out, emi_out, st));
      if (m.timing) HIPCHK(hipEventRecord(w.ev[2 + which], st));
    }
  }
  if (!far_only) {
    rc = add_outer(); // after the timing events: not part of the per-kernel times
    if (rc) return rc;
  }
  // a serial call reads table set 0 too: a later pipelined call, which prepares its set on far_st without waiting for
  // the caller's stream, must find the event behind THIS call's kernels
  rc = w.end_call(st, b);
  if (rc) return rc;
  w.pipelined = overlap != 0;
  w.timed = m.timing;
  w.counted = m.counting;
  return SR_OK;
}

// The coefficient op with the output weights of `W` (sr_kernels.hpp); the public entry points below
// choose W.  abs_out / emi_out: DEVICE [n_layers][g_hi - g_lo].
static int coef_op(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *abs_out,
                   double *emi_out, void *stream, const WeightMode W, const CoefOpt opt = CoefOpt()) {
  const bool far_only = opt.far_coef != nullptr;
  if (!far_only && (!abs_out || !emi_out)) return SR_ERR_ARG;
  int rc = check_coef_call(ls, atm, g_lo, g_hi);
  if (!rc) rc = check_line_shape(ls->parent ? ls->parent : ls, atm);
  if (rc) return rc;
  // one snapshot of the mode switches per call
  CoefModes m;
  m.variant = g_variant.load();
  m.timing = g_timing.load() != 0;
  const int far_mode = g_far_field.load();
  m.sparse_set = is_sparse_set(ls, far_mode);
  m.far_field = far_mode == 3 ? (m.sparse_set ? 1 : 2) : far_mode;
  if (far_only && !m.far_field) return SR_ERR_UNSUPPORTED; // (mc_pass takes the per-level route in the exact mode)
  m.counting = g_counting.load() != 0 && m.far_field;
  m.overlap = (g_overlap.load() != 0 && m.far_field && !m.counting) ? 1 : 0;
  const int rep_k = m.overlap ? -1 : g_repeat_kernel.load(), rep_n = g_repeat_n.load();
  for (int i = 0; i < 6; ++i) m.reps[i] = i == rep_k ? rep_n : 1;
  // layer batches under the table budget
  const size_t n_pts = (size_t)(g_hi - g_lo);
  const int nl_max = (int)std::max<size_t>(1, g_table_budget.load() / coef_bytes_per_layer(ls, n_pts, m.far_field, m.overlap));
  if (atm->n_layers > nl_max && far_only) {
    g_err = "far-only pass over more layers than the table budget holds (mc_pass sizes its row batches for the parent)";
    return SR_ERR_LIMIT;
  }
  return for_layer_batches(atm, ls->parent ? ls->parent : ls, ls->n_levels, true, nl_max, [&](const sr_layers_desc &sub, int k0) {
    return coef_batch(ls, &sub, g_lo, g_hi, abs_out + (size_t)k0 * n_pts, emi_out + (size_t)k0 * n_pts,
                      static_cast<hipStream_t>(stream), W, opt, m);
  });
}

// Sub-lineset of the lines whose upper or lower level is `level` (same grid, iso-molecule and level
// table), built on first use.  For the 'all' set (no levels) the lineset itself.
// up_only: only the lines whose upper level is `level` (sp_emission / ind_emission select those, spcl:1304-1313).
static int level_set(sr_lineset *ls, int level, sr_lineset **out, bool up_only = false) {
  if (level == -1) { // every line of the iso-molecule
    *out = ls;
    return SR_OK;
  }
  if (ls->n_levels == 0) {
    if (level != 0) return SR_ERR_ARG;
    *out = ls;
    return SR_OK;
  }
  if (level < 0 || level >= ls->n_levels) return SR_ERR_ARG;
  std::vector<sr_lineset *> &sets = up_only ? ls->level_up_sets : ls->level_sets;
  if (sets.empty()) sets.assign((size_t)ls->n_levels, nullptr);
  if (!sets[(size_t)level]) {
    sr_lineset *c = new sr_lineset();
    c->gp = ls->gp;
    c->mol = ls->mol;
    c->iso = ls->iso;
    c->mm = ls->mm;
    c->n_levels = ls->n_levels;
    c->e_lev = ls->e_lev;
    c->work = ls->work; // scratch, streams and events of the parent (see CoefWork)
    c->parent = ls;
    for (int which = 0; which < 2; ++which) {
      const HostLines &H = which ? ls->host_outer : ls->host;
      std::vector<int64_t> sel;
      for (int64_t q = 0; q < H.m; ++q)
        if (H.i[1 * H.md + q] == level || (!up_only && H.i[2 * H.md + q] == level)) sel.push_back(q);
      (which ? c->host_outer : c->host) = subset(H, sel);
    }
    const int rc = lineset_upload(c);
    if (rc) { sr_lineset_destroy(c); return rc; }
    sets[(size_t)level] = c;
  }
  *out = sets[(size_t)level];
  return SR_OK;
}

// Far pass f of a multi-channel pass: the level whose sub-lineset it runs over (ind: its ind_emission lines, those whose
// UPPER level is lv only), the weights of that sub-lineset's own coefficient op, and the channels its two outputs
// belong to (-1: none -- the unused second channel of the ind_emission weights)
struct McFarMap {
  int level, ch_a, ch_e;
  bool ind;
  WeightMode W;
};
static McFarMap mc_far_pass(int ctypes3, int f) {
  if (!ctypes3) return McFarMap{f, 2 * f, 2 * f + 1, false, WeightMode{kWeightLevelPair, f}};
  const int lv = f / 2;
  if (f & 1) return McFarMap{lv, 3 * lv + 1, -1, true, WeightMode{kWeightGind, lv}};
  return McFarMap{lv, 3 * lv + 2, 3 * lv, false, WeightMode{kWeightGabsGsp, lv}};
}

// What the row batches of one multi-channel pass share
struct McCall {
  sr_lineset *ls;
  int64_t g_lo, g_hi;
  double *out;
  void *stream;
  int ctypes3, far_mode, n_rows, n_far;
  McChannels mc;
  size_t coef_row; // doubles per (far pass, row)
  bool timing;
};

// The SPARSE sub-linesets of a row batch (is_sparse_set -- per-line expansions at every level,
// sr_farfield_rows_kernel): ALL of them in one batch of three launches -- tables, expansions, downward
// pass -- on the handle's near_st, beside the dense passes' chains.  One coefficient op each, they were eleven launches
// of 0.3 ms, latency-bound, each behind ~0.3 ms of host calls: 6 ms of a 13 ms build (gpurun_out/r06/tl_v4.txt).
// They share this pass's layer stage: their own would hold the same numbers (margins of the parent).
// far[f].coef of every sparse pass is set (nullptr: no line of it meets the shard); the others are left in `dense`.
static int mc_sparse_passes(const McCall &c, const LayerStage &S, const std::vector<sr_lineset *> &child, const std::vector<int> &order,
                            const std::vector<McFarMap> &pass, McFarPass *far, std::vector<int> *dense) {
  sr_lineset *ls = c.ls;
  McWork &m = ls->mc;
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  const int nl = S.A.n_layers;
  const size_t n_pts = (size_t)(c.g_hi - c.g_lo);
  int rc = m.s_batch.prepare(sizeof(FarBatchItem) * (size_t)c.n_far);
  if (rc) return rc;
  FarBatchItem *items = m.s_batch.host<FarBatchItem>();
  int n_items = 0, max_sub = 0;
  size_t rec_total = 0;
  std::vector<size_t> rec_off;
  for (int q = 0; q < c.n_far; ++q) {
    const int f = order[(size_t)q];
    sr_lineset *ch = child[(size_t)f];
    if (!is_sparse_set(ch, c.far_mode)) { dense->push_back(f); continue; }
    const IcIndex cx = shard_lines(ch, c.g_lo, c.g_hi);
    if (cx.n_sub <= 0) continue;
    FarBatchItem &it = items[n_items++];
    it.L = ch->L;
    it.first = cx.first;
    it.first_x0 = cx.x0;
    it.first_n = cx.n_tab;
    it.line_lo = cx.line_lo;
    it.n_sub = cx.n_sub;
    it.W = pass[(size_t)f].W;
    it.coef = m.d_coef.as<double>() + c.coef_row * (size_t)nl * f;
    far[f].coef = it.coef;
    rec_off.push_back(rec_total);
    rec_total += (size_t)cx.n_sub * nl;
    max_sub = std::max(max_sub, cx.n_sub);
  }
  m.batch_pending = n_items > 0;
  if (n_items <= 0) return SR_OK;
  rc = m.d_bfast.ensure(sizeof(FastRec) * (rec_total + 1));
  if (rc) return rc;
  for (int i = 0; i < n_items; ++i) items[i].fast = m.d_bfast.as<FastRec>() + rec_off[(size_t)i];
  // (serial schedule, sr_set_overlap(0): everything on the caller's stream, one kernel after the other)
  hipStream_t bst = st;
  if (g_overlap.load() != 0) { // beside the dense passes' chains (far_st): the handle's near_st
    hipStream_t fst = nullptr;
    rc = ls->work->pipeline_streams(&fst, &bst);
    if (rc) return rc;
  }
  if (bst != st) HIPCHK(hipStreamWaitEvent(bst, m.ev_prep, 0));
  rc = m.s_batch.push(sizeof(FarBatchItem) * (size_t)n_items, bst);
  if (rc) return rc;
  const double *l2l_tab = nullptr;
  rc = l2l_table_dev(&l2l_tab);
  if (rc) return rc;
  LAUNCHCHK(launch_far_batch(m.s_batch.d.as<FarBatchItem>(), n_items, max_sub, S.A, ls->gp, S.zmax, (int)c.g_lo,
                             far_params(n_pts, S, kFarPerLineRows, nullptr), l2l_tab, bst));
  HIPCHK(hipEventRecord(m.ev_zones, bst));
  return m.s_batch.mark(bst);
}

// One row batch [k0, k0 + sub.n_layers) of a multi-channel pass
static int mc_rows(const McCall &c, const sr_layers_desc &sub, int k0) {
  sr_lineset *ls = c.ls;
  CoefWork &w = *ls->work;
  McWork &m = ls->mc;
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  const int nl = sub.n_layers, n_far = c.n_far;
  const size_t n_pts = (size_t)(c.g_hi - c.g_lo);
  // this batch after everything earlier on the handle (the previous batch's kernels read the tables refilled below)
  if (w.last_done_recorded) HIPCHK(hipStreamWaitEvent(st, w.ev_last_done, 0));
  // (prepare() waits on the HOST for the mark behind the previous batch's -- or build's -- last kernel: nothing of this
  // batch is enqueued before the previous one has finished with the pass's scratch.  That is what keeps the far passes
  // below, whose internal streams are not ordered after the caller's, from writing m.d_coef under the wings kernel of
  // the batch before.)
  LayerStage S;
  int rc = stage_layers(m.s_layers, ls, ls, ls, &sub, 0.0, true, nullptr, st, &S);
  if (rc) return rc;
  const IcIndex ix = shard_lines(ls, c.g_lo, c.g_hi);
  const int line_lo = ix.line_lo, n_sub = ix.n_sub;
  auto chan_rows = [&](int ch) { return c.out + ((size_t)ch * c.n_rows + (size_t)k0) * n_pts; };
  std::vector<McFarMap> pass((size_t)n_far);
  for (int f = 0; f < n_far; ++f) pass[(size_t)f] = mc_far_pass(c.ctypes3, f);
  if (n_sub <= 0) {
    for (int ch = 0; ch < c.mc.n_ch; ++ch) HIPCHK(hipMemsetAsync(chan_rows(ch), 0, sizeof(double) * n_pts * nl, st));
  } else {
    rc = m.d_fast.ensure(sizeof(FastRec) * ((size_t)n_sub * nl + 1));
    if (!rc) rc = m.d_cold.ensure(sizeof(ColdRec) * ((size_t)n_sub * nl + 1));
    if (!rc) rc = m.d_coef.ensure(sizeof(double) * c.coef_row * (size_t)nl * n_far);
    if (rc) return rc;
    const ShardTables t{m.d_fast.as<FastRec>(), m.d_cold.as<ColdRec>(), ix, S.zmax, nl, (int)c.g_lo, (int)c.g_hi};
    if (c.timing) HIPCHK(hipEventRecord(m.ev_t[0], st));
    LAUNCHCHK(launch_prep(ls->L, S.A, ls->gp, WeightMode{kWeightChannels, c.ctypes3 ? 1 : 0}, line_lo, n_sub, (int)c.g_lo, (int)c.g_hi - 1,
                          m.d_fast.as<FastRec>(), m.d_cold.as<ColdRec>(), st));
    if (c.timing) HIPCHK(hipEventRecord(m.ev_t[1], st));
    HIPCHK(hipEventRecord(m.ev_prep, st)); // the layer stage, the tables and everything earlier on the caller's stream
    // The zones kernel beside the far passes, the wings kernel after both.  The build is bound by its kernels' WORK, not
    // their order -- 13.25 / 13.32 ms with the zones kernel gated behind the far passes, 13.06 / 13.13 beside them; the
    // sparse passes' single batched launch no longer starves beside it as their twelve small chains did
    // (profiles/r06_mc_timeline_v3 / v5).
    LAUNCHCHK(launch_zones_mc(t, ls->L.lev_up + line_lo, ls->L.lev_lo + line_lo, ls->gp, c.mc, c.out, c.n_rows, k0, st));
    if (c.timing) HIPCHK(hipEventRecord(m.ev_t[2], st));
    // far-only passes of the level sub-linesets
    rc = m.s_far.prepare(sizeof(McFarPass) * (size_t)n_far);
    if (rc) return rc;
    McFarPass *far = m.s_far.host<McFarPass>();
    // The passes are independent of each other.  The dense ones (one or two per build) go one after the other on the
    // handle's far_st, each through a CoefWork of its own (tables, events) instead of the handle's shared one, so that
    // none waits for another's scratch; the sparse ones in one batch beside them (mc_sparse_passes) -- one after the
    // other on one chain stream the eleven sparse passes (0.33 ms each, latency-bound) and the dense ground-state pass
    // were 7.7 ms, longer than the zones kernel they run beside.  Largest sub-lineset first (its chain is the longest).
    if (!m.fw_init) {
      for (auto &fwk : m.fw) {
        rc = fwk.init();
        if (rc) return rc;
        fwk.streams_of = &w; // the handle's two streams, not a set each
      }
      m.fw_init = true;
    }
    std::vector<sr_lineset *> child((size_t)n_far, nullptr);
    std::vector<int> order((size_t)n_far), dense;
    for (int f = 0; f < n_far; ++f) {
      rc = level_set(ls, pass[(size_t)f].level, &child[(size_t)f], pass[(size_t)f].ind);
      if (rc) return rc;
      order[(size_t)f] = f;
      far[f] = McFarPass{nullptr, pass[(size_t)f].ch_a, pass[(size_t)f].ch_e};
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return child[(size_t)x]->n_lines > child[(size_t)y]->n_lines; });
    rc = mc_sparse_passes(c, S, child, order, pass, far, &dense);
    if (rc) return rc;
    // the dense passes (the ground state's, typically), each through a CoefWork of its own
    for (size_t q = 0; q < dense.size(); ++q) {
      const int f = dense[q];
      sr_lineset *ch = child[(size_t)f];
      bool has = false;
      CoefOpt o;
      o.far_coef = m.d_coef.as<double>() + c.coef_row * (size_t)nl * f;
      o.far_has = &has;
      CoefWork *const shared = ch->work;
      ch->work = &m.fw[q % kMcFarLanes];
      rc = coef_op(ch, &sub, c.g_lo, c.g_hi, nullptr, nullptr, c.stream, pass[(size_t)f].W, o);
      ch->work = shared;
      if (rc) return rc;
      if (has) far[f].coef = o.far_coef;
    }
    if (m.batch_pending) HIPCHK(hipStreamWaitEvent(st, m.ev_zones, 0));
    rc = m.s_far.push(sizeof(McFarPass) * (size_t)n_far, st);
    if (rc) return rc;
    if (c.timing) HIPCHK(hipEventRecord(m.ev_t[3], st));
    LAUNCHCHK(launch_wings_mc(t, ls->L.lev_up + line_lo, ls->L.lev_lo + line_lo, far_params(n_pts, S, kFarPerLine, nullptr), c.mc,
                              m.s_far.d.as<McFarPass>(), n_far, c.out, c.n_rows, k0, st));
    if (c.timing) {
      HIPCHK(hipEventRecord(m.ev_t[4], st));
      m.timed = true;
    }
    rc = m.s_far.mark(st);
    if (rc) return rc;
  }
  // lines whose centre lies outside their window (humliv_bb's outer branches): per level, as the per-level route
  if (ls->n_outer > 0) {
    // (one record buffer for the largest level: sized per level, a growing buffer was freed -- a device synchronisation --
    // between the levels' launches)
    rc = m.d_outer_recs.ensure(sizeof(OuterRec) * (size_t)ls->n_outer * nl);
    if (rc) return rc;
    for (const McFarMap &p : pass) {
      sr_lineset *ch = nullptr;
      rc = level_set(ls, p.level, &ch, p.ind);
      if (rc) return rc;
      if (ch->n_outer <= 0) continue;
      double *o_e = p.ch_e >= 0 ? chan_rows(p.ch_e) : nullptr;
      if (!o_e) {
        rc = ls->d_gscratch.ensure(sizeof(double) * n_pts * nl); // the unused second channel of the ind_emission weights
        if (rc) return rc;
        o_e = ls->d_gscratch.as<double>();
      }
      LAUNCHCHK(launch_outer(ch->Lo, ch->n_outer, S.A, ls->gp, p.W, m.d_outer_recs.as<OuterRec>(), (int)c.g_lo, (int)c.g_hi,
                             chan_rows(p.ch_a), o_e, st));
    }
  }
  rc = m.s_layers.mark(st);
  if (rc) return rc;
  return w.end_call(st, -1);
}

// ------------------------------------------------------------------------
// The multi-channel pass: all level spectra of a (P, T) row stack from ONE walk of the full line list (near field:
// sr_zones_mc_kernel, sr_wings_mc_kernel) + one far-only pass per level sub-lineset (the far field is linear per output
// spectrum: its translations and polynomials cost the same per level whoever sums them).
//   ctypes3 = 0: out [n_levels][2][n_rows][n_pts], the pair tables of sr_glevel_pairs_dev
//   ctypes3 = 1: out [n_levels][3][n_rows][n_pts], sp_emission | ind_emission | absorption (sr_gcoeff_levels_dev)
// Returns SR_ERR_UNSUPPORTED (and does nothing) where the route does not apply -- exact mode, counting passes, more
// channels than an LDS image holds -- the callers then run one coefficient op per level.
// spect_main_module.py:1122-1168 (add_PT per level), spect_classes.py:1304-1321 (which lines a level owns).
// ------------------------------------------------------------------------
static int mc_pass(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *out, void *stream, int ctypes3) {
  const int nlev = ls->n_levels;
  McCall c{ls, g_lo, g_hi, out, stream, ctypes3, g_far_field.load(), atm->n_layers, ctypes3 ? 2 * nlev : nlev};
  if (nlev <= 0 || c.far_mode == 0 || g_counting.load() != 0 || g_level_route.load() == 0) return SR_ERR_UNSUPPORTED;
  int rc = check_coef_call(ls, atm, g_lo, g_hi);
  if (!rc) rc = check_line_shape(ls->parent ? ls->parent : ls, atm);
  if (rc) return rc;
  const McChannels &mc = c.mc = ctypes3 ? McChannels{3, 2, 0, 1, 3 * nlev} : McChannels{2, 0, 1, 0, 2 * nlev}; // stride, o_lo, o_up_e, o_up_a, n_ch
  if (mc.n_ch > 1023) return SR_ERR_UNSUPPORTED; // (10 bits per channel in the zones kernel's packed item word)
  if (zones_mc_image(mc.n_ch) == 0 || wings_mc_lds(mc.n_ch) > (size_t)160 * 1024) return SR_ERR_UNSUPPORTED;
  McWork &m = ls->mc;
  const size_t n_pts = (size_t)(g_hi - g_lo);
  FarParams fp0;
  far_hierarchy(n_pts, 1, &fp0);
  c.coef_row = (size_t)fp0.n_boxes_total * 2 * kFC;
  // row batches under the table budget
  const int rows_max = (int)std::max<size_t>(1, g_table_budget.load() / mc_bytes_per_row(ls, n_pts, c.coef_row, c.n_far));
  if (!m.ev_prep) {
    HIPCHK(hipEventCreateWithFlags(&m.ev_prep, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m.ev_zones, hipEventDisableTiming));
    for (auto &e : m.ev_t) HIPCHK(hipEventCreate(&e));
  }
  c.timing = g_timing.load() != 0; // (the events of the LAST row batch stay readable: sr_last_level_tables_ms)
  m.timed = false;
  return for_layer_batches(atm, ls, nlev, false, rows_max, [&](const sr_layers_desc &sub, int k0) { return mc_rows(c, sub, k0); });
}

extern "C" {

int sr_abscoeff_layers_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi,
                           double *abs_out, double *emi_out, void *stream) {
  return coef_op(ls, atm, g_lo, g_hi, abs_out, emi_out, stream, WeightMode{kWeightFolded, 0});
}

// ---- line strengths (spect_classes.py:208-310): HITRAN intensities, strengths per (layer, line), spectra weighted by them

int sr_lineset_set_strengths(sr_lineset *ls, const double *s_ref, int64_t n_lines, double t_ref, double q_ref,
                             double iso_ab) {
  if (!ls || ls->parent || (!s_ref && n_lines > 0)) return SR_ERR_ARG;
  if (n_lines != ls->n_in || !(t_ref > 0.0) || !std::isfinite(t_ref) || !(iso_ab > 0.0) || !std::isfinite(iso_ab) ||
      !std::isfinite(q_ref))
    return SR_ERR_ARG;
  for (int64_t i = 0; i < n_lines; ++i)
    if (!std::isfinite(s_ref[i])) return SR_ERR_ARG;
  // the previous set may still be read by calls in flight on this handle (every call records ev_last_done last)
  CoefWork &w = *ls->work;
  if (w.last_done_recorded) HIPCHK(hipEventSynchronize(w.ev_last_done));
  const size_t nm = ls->in_main.size(), no = ls->in_outer.size();
  std::vector<double> dev(std::max<size_t>(nm + no, 1), 0.0); // device order: main lines, then the outer ones
  for (size_t p = 0; p < nm; ++p) dev[p] = s_ref[ls->in_main[p]];
  for (size_t p = 0; p < no; ++p) dev[nm + p] = s_ref[ls->in_outer[p]];
  int rc = ls->d_sref.ensure(sizeof(double) * dev.size());
  if (rc) return rc;
  HIPCHK(hipMemcpy(ls->d_sref.p, dev.data(), sizeof(double) * dev.size(), hipMemcpyHostToDevice));
  ls->L.s_ref = ls->d_sref.as<double>();
  ls->Lo.s_ref = ls->d_sref.as<double>() + nm;
  ls->has_strengths = true;
  ls->s_t_ref = t_ref;
  ls->s_q_ref = q_ref;
  ls->s_iso_ab = iso_ab;
  return SR_OK;
}

// Q(t_ref) of the intensities: given, or CalcPartitionSum (SR_ERR_TABLE for an iso-molecule the tables lack)
static int strengths_q_ref(const sr_lineset *ls, double *q_ref) {
  if (ls->s_q_ref > 0.0) {
    *q_ref = ls->s_q_ref;
    return SR_OK;
  }
  return sr_calc_partition_sum(ls->mol, ls->iso, &ls->s_t_ref, 1, q_ref);
}

int sr_line_strengths_dev(sr_lineset *ls, const sr_layers_desc *atm, int source, double iso_ab, double *s_ab,
                          double *s_em, void *stream) {
  if (!ls || ls->parent || !atm || !s_ab) return SR_ERR_ARG;
  if (atm->n_layers <= 0 || atm->n_layers > 65535 || !atm->temps) return SR_ERR_ARG;
  if (source != SR_STRENGTH_EINSTEIN && source != SR_STRENGTH_HITRAN) return SR_ERR_ARG;
  if (source == SR_STRENGTH_EINSTEIN && !std::isfinite(iso_ab)) return SR_ERR_ARG;
  if (source == SR_STRENGTH_HITRAN && !ls->has_strengths) return SR_ERR_ARG;
  const int nl = atm->n_layers;
  for (int k = 0; k < nl; ++k)
    if (!(atm->temps[k] > 0.0)) return SR_ERR_ARG;
  if (atm->tvib)
    for (size_t i = 0; i < (size_t)ls->n_levels * nl; ++i)
      if (!(atm->tvib[i] > 0.0)) return SR_ERR_ARG;
  double q_ref = 0.0;
  if (source == SR_STRENGTH_HITRAN) {
    const int rc = strengths_q_ref(ls, &q_ref);
    if (rc) return rc;
  }
  if (ls->n_in == 0) return SR_OK;
  // fill_layer_stage reads the pressures for the coefficient op's margins only
  std::vector<double> press(nl, 0.0);
  sr_layers_desc a = *atm;
  if (!a.press) a.press = press.data();
  hipStream_t st = static_cast<hipStream_t>(stream);
  CoefWork &w = *ls->work;
  LayerStage S;
  int rc = stage_layers(ls->s_str, ls, ls, ls, &a, source == SR_STRENGTH_HITRAN ? q_ref : 0.0, false,
                        w.last_done_recorded ? w.ev_last_done : nullptr, st, &S);
  if (rc) return rc;
  LAUNCHCHK(launch_line_strengths(ls->L, ls->Lo, ls->d_inpos.as<int>(), (int)ls->n_in, S.A, source, iso_ab, ls->s_t_ref,
                                  s_ab, s_em, st));
  rc = ls->s_str.mark(st);
  if (rc) return rc;
  return w.end_call(st, -1);
}

int sr_abscoeff_layers_from_strengths_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi,
                                          double *abs_out, double *emi_out, void *stream) {
  if (!ls || ls->parent || !ls->has_strengths) return SR_ERR_ARG;
  if (ls->linear_weights) {
    g_err = "the strength weights have no linearised form (sr_lineset_set_linear_weights)";
    return SR_ERR_UNSUPPORTED;
  }
  CoefOpt opt;
  int rc = strengths_q_ref(ls, &opt.q_ref);
  if (rc) return rc;
  WeightMode W{kWeightStrength, 0};
  W.t_ref = ls->s_t_ref;
  W.inv_iso_ab = 1.0 / ls->s_iso_ab;
  return coef_op(ls, atm, g_lo, g_hi, abs_out, emi_out, stream, W, opt);
}

int sr_gcoeff_layers_dev(sr_lineset *ls, const sr_layers_desc *atm, int level, int64_t g_lo, int64_t g_hi,
                         double *g_out, void *stream) {
  if (!g_out || check_coef_call(ls, atm, g_lo, g_hi, true)) return SR_ERR_ARG;
  if (const int rcs = check_line_shape(ls->parent ? ls->parent : ls, atm)) return rcs; // before any sub-lineset is cut
  sr_lineset *c = nullptr;
  int rc = level_set(ls, level, &c);
  if (rc) return rc;
  const size_t plane = (size_t)atm->n_layers * (size_t)(g_hi - g_lo);
  rc = ls->d_gscratch.ensure(sizeof(double) * plane); // the parent's: one for all levels
  if (rc) return rc;
  // pass 1: abs channel = absorption (lines whose LOWER level is `level`), emi channel = sp_emission
  // (UPPER level); pass 2: abs channel = ind_emission (UPPER level), emi channel unused
  const int wl = ls->n_levels == 0 ? -1 : level; // no level table: lev_up = lev_lo = 0 for every line anyway
  rc = coef_op(c, atm, g_lo, g_hi, g_out + 2 * plane, g_out + 0 * plane, stream, WeightMode{kWeightGabsGsp, wl});
  if (rc) return rc;
  // ind_emission selects the lines whose UPPER level is `level`: the second pass runs on those alone (round 4; for
  // the ground level, which 80 % of a hot-band list have as their lower level, that is an empty set instead of
  // the whole list a second time)
  sr_lineset *cu = nullptr;
  rc = level_set(ls, level, &cu, true);
  if (rc) return rc;
  return coef_op(cu, atm, g_lo, g_hi, g_out + 1 * plane, ls->d_gscratch.as<double>(), stream,
                 WeightMode{kWeightGind, wl});
}

int sr_abscoeff_level_dev(sr_lineset *ls, const sr_layers_desc *atm, int level, int64_t g_lo, int64_t g_hi,
                          double *abs_out, double *emi_out, void *stream) {
  if (!ls) return SR_ERR_ARG;
  sr_lineset *c = nullptr;
  const int rc = level_set(ls, level, &c);
  if (rc) return rc;
  return coef_op(c, atm, g_lo, g_hi, abs_out, emi_out, stream, WeightMode{kWeightTracked, level});
}

int sr_glevel_pairs_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *out, void *stream) {
  if (!out || check_coef_call(ls, atm, g_lo, g_hi, true)) return SR_ERR_ARG;
  if (const int rcs = check_line_shape(ls->parent ? ls->parent : ls, atm)) return rcs; // before any sub-lineset is cut
  const size_t plane = (size_t)atm->n_layers * (size_t)(g_hi - g_lo);
  if (ls->n_levels == 0) // the 'all' set: every line, pop = 1 / Q in the combine (smm:2052-2057)
    return coef_op(ls, atm, g_lo, g_hi, out, out + plane, stream, WeightMode{kWeightLevelPair, -1});
  {
    // every line once, its three weights to the spectra of its two levels (mc_pass); where that route does not apply
    // (exact mode, counting, sr_set_level_route(0)): one coefficient op per level, below
    const int rc = mc_pass(ls, atm, g_lo, g_hi, out, stream, 0);
    if (rc != SR_ERR_UNSUPPORTED) return rc;
  }
  for (int lv = 0; lv < ls->n_levels; ++lv) {
    sr_lineset *c = nullptr;
    int rc = level_set(ls, lv, &c); // lines whose upper or lower level is lv
    if (rc) return rc;
    rc = coef_op(c, atm, g_lo, g_hi, out + (size_t)(2 * lv) * plane, out + (size_t)(2 * lv + 1) * plane, stream,
                 WeightMode{kWeightLevelPair, lv});
    if (rc) return rc;
  }
  return SR_OK;
}

int sr_gcoeff_levels_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *g_out, void *stream) {
  if (!g_out || check_coef_call(ls, atm, g_lo, g_hi, true)) return SR_ERR_ARG;
  if (const int rcs = check_line_shape(ls->parent ? ls->parent : ls, atm)) return rcs; // before any sub-lineset is cut
  if (ls->n_levels == 0) return sr_gcoeff_layers_dev(ls, atm, 0, g_lo, g_hi, g_out, stream);
  {
    const int rc = mc_pass(ls, atm, g_lo, g_hi, g_out, stream, 1);
    if (rc != SR_ERR_UNSUPPORTED) return rc;
  }
  const size_t plane3 = 3 * (size_t)atm->n_layers * (size_t)(g_hi - g_lo);
  for (int lv = 0; lv < ls->n_levels; ++lv) {
    const int rc = sr_gcoeff_layers_dev(ls, atm, lv, g_lo, g_hi, g_out + plane3 * (size_t)lv, stream);
    if (rc) return rc;
  }
  return SR_OK;
}

int sr_glevel_combine_dev(const double *tab, const double *tab_dT, int n_levels, int n_rows, int64_t n_pts, int n_steps,
                          const int32_t *step_row, const double *pop, const double *dpop, double inv_dT,
                          double *abs_out, double *emi_out, double *dabs_out, double *demi_out, void *stream) {
  if (!tab || !step_row || !pop || !abs_out || !emi_out || n_levels <= 0 || n_rows <= 0 || n_pts <= 0 || n_steps <= 0)
    return SR_ERR_ARG;
  if (n_levels > SR_MAX_LEVELS || n_pts > 2000000) return SR_ERR_LIMIT;
  if (tab_dT && (!dpop || !dabs_out || !demi_out || !(inv_dT == inv_dT))) return SR_ERR_ARG;
  for (int s = 0; s < n_steps; ++s)
    if (step_row[s] < 0 || step_row[s] >= n_rows) return SR_ERR_ARG; // would read out of the tables
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the steps grouped by table row (counting sort: the order of the steps inside a row is the caller's)
  std::vector<int> count((size_t)n_rows + 1, 0);
  for (int s = 0; s < n_steps; ++s) ++count[(size_t)step_row[s] + 1];
  std::vector<int> rows_used, row_off(1, 0), start((size_t)n_rows, 0);
  for (int r = 0; r < n_rows; ++r)
    if (count[(size_t)r + 1] > 0) {
      start[(size_t)r] = row_off.back();
      rows_used.push_back(r);
      row_off.push_back(row_off.back() + count[(size_t)r + 1]);
    }
  std::vector<int> step_of((size_t)n_steps), fill(start);
  for (int s = 0; s < n_steps; ++s) step_of[(size_t)fill[(size_t)step_row[s]]++] = s;
  const int n_used = (int)rows_used.size();
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const size_t n_pop = (size_t)n_steps * n_levels;
  const auto p_pop = pk.copy(pop, n_pop), p_dpop = pk.copy(dpop, tab_dT ? n_pop : 0);
  const auto p_used = pk.copy(rows_used.data(), rows_used.size()), p_off = pk.copy(row_off.data(), row_off.size());
  const auto p_step = pk.copy(step_of.data(), step_of.size());
  const int rc = pk.stage(st);
  if (rc) return rc;
  LAUNCHCHK(launch_glevel_combine(tab, tab_dT, n_levels, n_rows, (int)n_pts, n_used, pk.dev(p_used), pk.dev(p_off), pk.dev(p_step),
                                  pk.dev(p_pop), pk.dev(p_dpop), inv_dT, abs_out, emi_out, dabs_out, demi_out, st));
  return pk.slot().mark(st);
}

int sr_abscoeff_layers(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi,
                       double *abs_out, double *emi_out) {
  if (!ls || !atm || !abs_out || !emi_out || g_lo >= g_hi || atm->n_layers <= 0) return SR_ERR_ARG;
  const size_t bytes = sizeof(double) * (size_t)(g_hi - g_lo) * atm->n_layers;
  DevBuf a, e;
  int rc = a.ensure(bytes);
  if (!rc) rc = e.ensure(bytes);
  if (!rc) rc = sr_abscoeff_layers_dev(ls, atm, g_lo, g_hi, a.as<double>(), e.as<double>(), nullptr);
  if (!rc) {
    hipError_t er = hipMemcpy(abs_out, a.p, bytes, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(emi_out, e.p, bytes, hipMemcpyDeviceToHost);
    if (er != hipSuccess) rc = hip_fail(er, "copy back");
  }
  a.release();
  e.release();
  return rc;
}

int sr_last_eval_counts(sr_lineset *ls, uint64_t *counts10) {
  uint64_t *counts8 = counts10;
  static_assert(kCntN == 10, "sr_last_eval_counts: the header documents ten counters");
  if (!ls || !counts8 || !ls->work->counted) return SR_ERR_ARG;
  HIPCHK(hipEventSynchronize(ls->work->ev_last_done));
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
  HIPCHK(hipMemcpy(counts8, ls->work->d_counts.p, sizeof(uint64_t) * kCntN, hipMemcpyDeviceToHost));
  return SR_OK;
}

int sr_last_kernel_ms(sr_lineset *ls, float *ms5) {
  if (!ls || !ls->work->timed || !ms5) return SR_ERR_ARG;
  HIPCHK(hipEventSynchronize(ls->work->ev[ls->work->n_timed]));
  for (int i = 0; i < 5; ++i) ms5[i] = 0.f;
  // ev[1] (end of prep) is on the prep stream when the call was pipelined: the kernels that follow
  // are measured from ev_op0, recorded on the caller's stream once it has the tables
  hipEvent_t first = ls->work->pipelined ? ls->work->ev_op0 : ls->work->ev[1];
  HIPCHK(hipEventElapsedTime(&ms5[0], ls->work->ev[0], ls->work->ev[1]));
  if (ls->work->overlapped) { // kernels run side by side: only the whole coefficient op has a duration
    HIPCHK(hipEventElapsedTime(&ms5[1], first, ls->work->ev[4]));
    return SR_OK;
  }
  for (int i = 1; i < ls->work->n_timed; ++i)
    HIPCHK(hipEventElapsedTime(&ms5[i], i == 1 ? first : ls->work->ev[i], ls->work->ev[i + 1]));
  return SR_OK;
}

int sr_last_level_tables_ms(sr_lineset *ls, float *ms4) {
  if (!ls || !ms4 || !ls->mc.timed) return SR_ERR_ARG;
  const McWork &m = ls->mc;
  HIPCHK(hipEventSynchronize(m.ev_t[4]));
  HIPCHK(hipEventElapsedTime(&ms4[0], m.ev_t[0], m.ev_t[1])); // tables of the full list
  HIPCHK(hipEventElapsedTime(&ms4[1], m.ev_t[1], m.ev_t[2])); // sr_zones_mc_kernel (beside the far passes unless the schedule is serial)
  HIPCHK(hipEventElapsedTime(&ms4[2], m.ev_t[2], m.ev_t[3])); // what of the far passes was left when it ended
  HIPCHK(hipEventElapsedTime(&ms4[3], m.ev_t[3], m.ev_t[4])); // sr_wings_mc_kernel
  return SR_OK;
}

} // extern "C"

namespace {

// The coefficient tables and the grid of a radiance or limb call; rest_ok: the call's other plain argument conditions,
// which rank with the pointers (SR_ERR_ARG) before the grid limit.
int check_limb_call(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, bool rest_ok) {
  if (!abs_c || !emi_c || n_layers <= 0 || n_pts <= 0 || !rest_ok) return SR_ERR_ARG;
  if (n_pts > 2000000) return SR_ERR_LIMIT;
  return SR_OK;
}

// The caller's segment lists of the sr_radiance_*_dev calls.  need_segments: the Jacobian calls refuse a batch
// without any segment.
int check_segments(int n_layers, int n_rays, const int32_t *seg_off, const int32_t *seg_layer, const double *seg_col,
                   bool need_segments, int *n_seg_out) {
  const int n_seg = seg_off[n_rays];
  if (seg_off[0] != 0 || n_seg < (need_segments ? 1 : 0)) return SR_ERR_ARG;
  if (n_seg > 0 && (!seg_layer || !seg_col)) return SR_ERR_ARG;
  for (int r = 0; r < n_rays; ++r)
    if (seg_off[r + 1] < seg_off[r]) return SR_ERR_ARG;
  for (int s = 0; s < n_seg; ++s)
    if (seg_layer[s] < 0 || seg_layer[s] >= n_layers) return SR_ERR_ARG; // would read out of bounds
  *n_seg_out = n_seg;
  return SR_OK;
}

// Their staged block -- the three segment arrays and, for the column Jacobian, d col / d par (n_dcol values, or 0) --
// sent up on a slot of the caller's ring, handed to the caller's launch(seg_off, seg_layer, seg_col, dcol) as device
// pointers, and the slot marked behind that kernel (it is refilled only after it: the copy does not ride on `st`)
template <class Launch>
int with_staged_segments(Stager &slot, int n_rays, int n_seg, const int32_t *seg_off, const int32_t *seg_layer,
                         const double *seg_col, const double *dcol, size_t n_dcol, hipStream_t st, Launch launch) {
  StagePack pk(slot);
  const auto p_off = pk.copy(seg_off, (size_t)n_rays + 1), p_layer = pk.copy(seg_layer, (size_t)n_seg, 1);
  const auto p_col = pk.copy(seg_col, (size_t)n_seg, 1), p_dcol = pk.copy(dcol, n_dcol);
  const int rc = pk.stage(st);
  if (rc) return rc;
  LAUNCHCHK(launch(pk.dev(p_off), pk.dev(p_layer), pk.dev(p_col), pk.dev(p_dcol)));
  return slot.mark(st);
}

} // namespace

extern "C" {

// ------------------------------------------------------------------------
int sr_radiance_rays_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, int n_rays,
                         const int32_t *seg_off, const int32_t *seg_layer, const double *seg_col,
                         int init_from_rad, double *rad, void *stream) {
  int n_seg = 0;
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, rad && seg_off && n_rays > 0);
  if (!rc) rc = check_segments(n_layers, n_rays, seg_off, seg_layer, seg_col, /*need_segments=*/false, &n_seg);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  static thread_local StagerRing ring;
  return with_staged_segments(ring.take(), n_rays, n_seg, seg_off, seg_layer, seg_col, nullptr, 0, st,
                              [&](const int *off, const int *layer, const double *col, const double *) {
    return launch_radiance(abs_c, emi_c, (int)n_pts, n_rays, off, layer, col, init_from_rad, rad, st);
  });
}

// ------------------------------------------------------------------------
int sr_radiance_jac_layer_dev(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                              int n_layers, int64_t n_pts, int n_rays, const int32_t *seg_off,
                              const int32_t *seg_layer, const double *seg_col, double *jac, void *stream) {
  int n_seg = 0;
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, dabs && demi && jac && seg_off && n_rays > 0);
  if (!rc) rc = check_segments(n_layers, n_rays, seg_off, seg_layer, seg_col, /*need_segments=*/true, &n_seg);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  static thread_local StagerRing ring;
  return with_staged_segments(ring.take(), n_rays, n_seg, seg_off, seg_layer, seg_col, nullptr, 0, st,
                              [&](const int *off, const int *layer, const double *col, const double *) {
    return launch_radiance_jac_layer(abs_c, emi_c, dabs, demi, (int)n_pts, n_layers, n_rays, off, layer, col, jac, st);
  });
}

// ------------------------------------------------------------------------
int sr_radiance_jac_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, int n_rays,
                        const int32_t *seg_off, const int32_t *seg_layer, const double *seg_col,
                        const double *dcol_dpar, int n_par, double *rad, double *jac, void *stream) {
  int n_seg = 0;
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, rad && jac && seg_off && dcol_dpar && n_rays > 0 && n_par > 0);
  if (!rc) rc = check_segments(n_layers, n_rays, seg_off, seg_layer, seg_col, /*need_segments=*/true, &n_seg);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  static thread_local StagerRing ring;
  return with_staged_segments(ring.take(), n_rays, n_seg, seg_off, seg_layer, seg_col, dcol_dpar, (size_t)n_seg * n_par, st,
                              [&](const int *off, const int *layer, const double *col, const double *dcol) {
    return launch_radiance_jac(abs_c, emi_c, (int)n_pts, n_rays, off, layer, col, dcol, n_par, rad, jac, st);
  });
}

// ------------------------------------------------------------------------
// Device LOS pipeline
// ------------------------------------------------------------------------
} // extern "C"

namespace {

// One staged LOS description on the device (a slot of a small ring, see sr_radiance_rays_dev).
struct LosDev {
  const int *seg_off, *seg_layer, *pt_off, *par_gas;
  const double *x, *nd, *prof, *scale;
  double *col;  // [n_gas + n_par][n_seg]
  int n_seg, n_pt, n_prof;
  Stager *slot;
};

// The entry points that start every ray from 0 or from the Planck function refuse an initial intensity read from a
// buffer, each with the status it has always answered.
int refuse_init_mode_1(const sr_los_desc *los, const char *entry, int status) {
  if (los->init_mode != 1) return SR_OK;
  g_err = std::string(entry) + ": init_mode 1 (intensity read from a buffer) is not supported, use 0 or 2";
  return status;
}

// Stage a checked LOS (check_los_par: `shape`) and evaluate the columns of the gases and of n_par profile parameters;
// `st` waits for them.  own: the staging slot of a device-resident LOS (sr_los_create) instead of the per-call ring.
// path (photon order only, the caller has checked): the sample points' derivatives to the ray's tangent altitude join
// the pack, and n_gas more rows behind the column table, rows n_gas + n_par .., take d col_g / d z_t
// (sr_los_columns_dz_kernel).
int stage_los(const sr_los_desc *los, const LosShape &shape, int n_par, const int32_t *par_gas, const double *par_w,
              hipStream_t st, LosDev *out, Stager *own = nullptr, const sr_los_path *path = nullptr) {
  static thread_local StagerRing ring;
  StagePack pk(own ? *own : ring.take());
  const int n_seg = shape.n_seg, n_pt = shape.n_pt, n_prof = los->n_gas + n_par, nr = los->n_rays;
  // (observer order re-lists x, nd, seg_layer and pt_off below)
  const auto p_x = pk.copy(los->x, (size_t)n_pt), p_nd = pk.copy(los->nd, (size_t)n_pt);
  const auto p_prof = pk.room<double>((size_t)n_prof * n_pt), p_scale = pk.room<double>((size_t)n_prof);
  const auto p_soff = pk.copy(los->seg_off, (size_t)nr + 1), p_slay = pk.copy(los->seg_layer, (size_t)n_seg);
  const auto p_poff = pk.copy(los->pt_off, (size_t)n_seg + 1), p_pgas = pk.copy(par_gas, (size_t)n_par, 1);
  StagePack::Part<double> p_alt{0}, p_dx{0}, p_dalt{0}; // (registered with a path only: the pack without is what it was)
  if (path) p_alt = pk.copy(path->alt, (size_t)n_pt), p_dx = pk.copy(path->dx_dz, (size_t)n_pt), p_dalt = pk.copy(path->dalt_dz, (size_t)n_pt);
  pk.tail(sizeof(double) * (size_t)(n_prof + (path ? los->n_gas : 0)) * n_seg); // the column table
  int rc = pk.prepare();
  if (rc) return rc;
  double *prs = pk.host(p_prof), *sc = pk.host(p_scale);
  std::memcpy(prs, los->vmr, sizeof(double) * (size_t)los->n_gas * n_pt);
  if (n_par) std::memcpy(prs + (size_t)los->n_gas * n_pt, par_w, sizeof(double) * (size_t)n_par * n_pt);
  for (int g = 0; g < los->n_gas; ++g) sc[g] = los->col_scale ? los->col_scale[g] : 1.0;
  for (int p = 0; p < n_par; ++p) sc[los->n_gas + p] = sc[par_gas[p]];
  // observer order: the recursion walks every ray's segments backwards.  Segment s keeps its index (and
  // its sample points, whose x must stay increasing); only the walk order changes, through a permutation
  // applied to seg_layer and to the column table's segment axis alike.
  std::vector<int> perm(n_seg);
  for (int r = 0; r < nr; ++r)
    for (int s = los->seg_off[r]; s < los->seg_off[r + 1]; ++s)
      perm[s] = los->los_order == 0 ? s : los->seg_off[r] + (los->seg_off[r + 1] - 1 - s);
  if (los->los_order != 0) {
    // re-list the segments in photon order: new segment q = old segment perm[q]; sample points re-packed
    std::vector<double> x2(n_pt), nd2(n_pt), pr2((size_t)n_prof * n_pt);
    int *sl = pk.host(p_slay), *po = pk.host(p_poff);
    int at = 0;
    for (int q = 0; q < n_seg; ++q) {
      const int s = perm[q], a = los->pt_off[s], b = los->pt_off[s + 1];
      sl[q] = los->seg_layer[s];
      po[q] = at;
      for (int i = a; i < b; ++i, ++at) {
        x2[at] = los->x[i];
        nd2[at] = los->nd[i];
        for (int f = 0; f < n_prof; ++f) pr2[(size_t)f * n_pt + at] = prs[(size_t)f * n_pt + i];
      }
    }
    po[n_seg] = at;
    std::memcpy(pk.host(p_x), x2.data(), sizeof(double) * n_pt);
    std::memcpy(pk.host(p_nd), nd2.data(), sizeof(double) * n_pt);
    std::memcpy(prs, pr2.data(), sizeof(double) * (size_t)n_prof * n_pt);
  }
  hipStream_t cs = nullptr;
  rc = pk.begin_early(&cs);
  if (rc) return rc;
  *out = LosDev{pk.dev(p_soff), pk.dev(p_slay), pk.dev(p_poff), pk.dev(p_pgas), pk.dev(p_x), pk.dev(p_nd), pk.dev(p_prof),
                pk.dev(p_scale), pk.dev_tail<double>(), n_seg, n_pt, n_prof, &pk.slot()};
  LAUNCHCHK(launch_los_columns(out->nd, out->x, out->prof, out->scale, out->pt_off, n_seg, n_pt, n_prof, out->col, cs));
  if (path)
    LAUNCHCHK(launch_los_columns_dz(out->nd, out->x, out->prof, out->scale, out->pt_off, pk.dev(p_alt), pk.dev(p_dx),
                                    pk.dev(p_dalt), n_seg, n_pt, los->n_gas, out->col + (size_t)n_prof * n_seg, cs));
  return pk.slot().end_early(cs, st);
}

// behind the kernels that read two staged blocks
int mark_both(Stager &a, Stager &b, hipStream_t st) {
  const int rc = a.mark(st);
  return rc ? rc : b.mark(st);
}

LimbOpts limb_opts(const sr_los_desc *los, int n_seg) {
  LimbOpts o;
  o.n_gas = los->n_gas;
  o.n_seg_total = n_seg;
  o.solo_absorption = los->solo_absorption ? 1 : 0;
  o.init_mode = los->init_mode;
  o.g_lo = (int)los->g_lo;
  o.t_init = los->t_init;
  o.w0 = los->w0;
  o.gstep = los->step;
  return o;
}

} // namespace

namespace {

// The folded kernels' plan on the device: per ray and visited shell (outermost first) the layer and the ray's two
// segments there, + room for the packed records.  n_rec = 0: some ray is not V-shaped, or the batch has more than
// kFoldGasMax gases (nothing staged).
struct FoldStage {
  const int *plan = nullptr;
  FoldDense *rec = nullptr;
  int n_vis = 0, n_rec = 0;
  Stager *slot = nullptr;
};
int stage_fold(const sr_los_desc *los, int n_layers, hipStream_t st, FoldStage *out, Stager *own = nullptr) {
  if (los->n_gas > kFoldGasMax) return SR_OK; // (the folded records hold four columns: such batches keep the path-order kernels)
  std::vector<int> far, near;
  int l_min = 0, l_max = -1;
  if (!fold_sides(los, n_layers, nullptr, &far, &near, &l_min, &l_max)) return SR_OK;
  const int nr = los->n_rays;
  const std::vector<int> shells = fold_shells(far, near, nr, n_layers, l_min, l_max);
  if ((size_t)nr * shells.size() > ((size_t)1 << 21)) return SR_OK; // (2M records = 436 MB of plan: such batches keep the path-order kernels)
  // The fold pays when the rays SHARE shells.  A 3-D batch lists a row per LOS step (seg_layer = arange): every ray then
  // looks like a slant ray through rows of its own, the union of the shells is the steps of ALL rays and a ray's plan is
  // mostly empty visits (n_rays x n_seg_total records).  Such batches keep the path-order kernel: the union may be at
  // most twice the shells of the longest ray.
  size_t longest = 0;
  for (int r = 0; r < nr; ++r) {
    size_t n_real = 0;
    for (int k : shells) n_real += far[(size_t)r * n_layers + k] >= 0 || near[(size_t)r * n_layers + k] >= 0;
    longest = std::max(longest, n_real);
  }
  if (shells.size() > 2 * longest) return SR_OK;
  const int n_vis = (int)shells.size(), n_rec = nr * n_vis;
  static thread_local StagerRing ring;
  StagePack pk(own ? *own : ring.take());
  const auto p_plan = pk.room<int>(4 * (size_t)n_rec);
  pk.tail(fold_dense_bytes(n_rec));
  int rc = pk.prepare();
  if (rc) return rc;
  int *pl = pk.host(p_plan);
  for (int r = 0; r < nr; ++r)
    for (int v = 0; v < n_vis; ++v) {
      int *q = pl + ((size_t)r * n_vis + v) * 4;
      q[0] = shells[v];
      q[1] = far[(size_t)r * n_layers + shells[v]];
      q[2] = near[(size_t)r * n_layers + shells[v]];
      q[3] = 0;
    }
  rc = pk.push_early(st);
  if (rc) return rc;
  *out = FoldStage{pk.dev(p_plan), pk.dev_tail<FoldDense>(), n_vis, n_rec, &pk.slot()};
  return SR_OK;
}

} // namespace

extern "C" {

int sr_los_columns(const sr_los_desc *los, double *col_out) {
  if (!col_out) return SR_ERR_ARG;
  LosShape shape;
  int rc = check_los(los, 0, &shape, kLimbGasMax);
  if (rc) return rc;
  LosDev D;
  rc = stage_los(los, shape, 0, nullptr, nullptr, nullptr, &D);
  if (rc) return rc;
  std::vector<double> tmp((size_t)los->n_gas * D.n_seg);
  HIPCHK(hipMemcpy(tmp.data(), D.col, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
  // back to the caller's segment numbering
  for (int g = 0; g < los->n_gas; ++g)
    for (int r = 0; r < los->n_rays; ++r)
      for (int s = los->seg_off[r]; s < los->seg_off[r + 1]; ++s) {
        const int q = los->los_order == 0 ? s : los->seg_off[r] + (los->seg_off[r + 1] - 1 - s);
        col_out[(size_t)g * D.n_seg + s] = tmp[(size_t)g * D.n_seg + q];
      }
  return SR_OK;
}

int sr_los_columns_dz(const sr_los_desc *los, const sr_los_path *path, double *dcol_out) {
  if (!dcol_out || !path || !path->alt || !path->dx_dz || !path->dalt_dz) return SR_ERR_ARG;
  LosShape shape;
  int rc = check_los(los, 0, &shape, kLimbGasMax);
  if (rc) return rc;
  if (los->los_order != 0) {
    g_err = "sr_los_columns_dz: the pointing derivative needs the batch in photon order (observer order re-lists the sample points)";
    return SR_ERR_UNSUPPORTED;
  }
  LosDev D;
  rc = stage_los(los, shape, 0, nullptr, nullptr, nullptr, &D, nullptr, path);
  if (rc) return rc;
  HIPCHK(hipMemcpy(dcol_out, D.col + (size_t)los->n_gas * D.n_seg, sizeof(double) * (size_t)los->n_gas * D.n_seg,
                   hipMemcpyDeviceToHost));
  return SR_OK;
}

static thread_local int g_last_limb_route = 0;
int sr_last_limb_route(void) { return g_last_limb_route; }
static thread_local int g_last_state_route = 0;     // limb_jac_state: 1 the dense plan, 2 parameter blocks per ray
static thread_local int64_t g_last_state_walks = 0; // its (ray, block) pairs
int sr_last_state_route(void) { return g_last_state_route; }
int64_t sr_last_state_walks(void) { return g_last_state_walks; }
int sr_last_state_instance(int32_t out[8]) {
  const sr::StateInstance &I = sr::g_last_state_instance;
  if (!out || I.ng == 0) return SR_ERR_ARG;
  const int32_t v[8] = {I.ng, I.np, I.cols, I.rows, I.bands, I.instr, I.several, I.rayblk};
  std::copy(v, v + 8, out);
  return SR_OK;
}

} // extern "C"

namespace sr {
thread_local StateInstance g_last_state_instance{}; // (sr_kernels.hpp: every state unit writes it)
}

// A LOS batch resident on the device (sr_los_create): the staged description, its Curtis-Godson columns and -- where
// the rays share their shells -- the folded sweep's packed records, all made ONCE.  The reference computes a LOS's
// steps once too (los.calc_radtran_steps, spect_main_module.py:2746-2767) and runs radtran on them many times.
struct sr_los {
  static constexpr const char *kName = "sr_los";
  Stager s_los, s_fold, s_vmr, s_x;
  LosDev D{};
  FoldStage F{};
  sr_los_desc opt{}; // the scalar options; its pointers are not kept
  int n_layers = 0, dev = -1;
  int n_par = 0;                 // column parameters staged with the batch (sr_los_create_par)
  std::vector<int32_t> par_gas;  // their gases (host copy: a kernel argument of the folded kernel)
  // The handle's device state (profiles, columns, packed records) is rewritten by set_vmr / refresh_columns /
  // retrieval_forward on whatever stream the caller passes: every entry point orders its stream after the handle's
  // last use (as coef_op does with ev_last_done), so calls on streams that are not ordered against each other are safe
  hipEvent_t ev_last = nullptr;
  bool last_recorded = false;
  hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr; // around the recursion of the last forward model (sr_set_timing(2))
  bool k_timed = false;
};

// Every call on a resident batch works inside one LosScope (a HandleScope; sr_abs_table's calls use the same scope).
// enter(): the handle belongs to the device it was made on
// (its buffers, and the pinned stagers that would rebuild themselves on another current device and then copy into this
// one's memory), and `st` waits for the handle's last use.  leave() records that use behind the call's work on `st` and
// returns the status; a call that returns early after enter() -- a failed launch or copy with work already enqueued on
// the handle -- leaves through the destructor, which records it all the same.
template <class H> class HandleScope {
 public:
  HandleScope(H *h, hipStream_t st) : h_(h), st_(st) {}
  ~HandleScope() {
    if (open_) (void)record();
  }
  int enter() {
    int cur = -1;
    HIPCHK(hipGetDevice(&cur));
    if (cur != h_->dev) {
      g_err = std::string(H::kName) + " handle used on device " + std::to_string(cur) + ", made on device " + std::to_string(h_->dev);
      return SR_ERR_ARG;
    }
    if (h_->last_recorded) HIPCHK(hipStreamWaitEvent(st_, h_->ev_last, 0));
    open_ = true;
    return SR_OK;
  }
  int leave() {
    HIPCHK(record());
    return SR_OK;
  }

 private:
  hipError_t record() {
    open_ = false;
    hipError_t e = h_->ev_last ? hipSuccess : hipEventCreateWithFlags(&h_->ev_last, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(h_->ev_last, st_);
    h_->last_recorded = h_->last_recorded || e == hipSuccess;
    return e;
  }
  H *h_;
  hipStream_t st_;
  bool open_ = false;
};
using LosScope = HandleScope<sr_los>;

// ------------------------------------------------------------------------
// The instrument step's per-thread device state (sr_hires_to_lowres_shard_dev, and sr_retrieval_forward_dev whose
// recursion kernel integrates the bands itself).
// The weight table depends on the grid window and the bands alone: kept while they (and the buffer) stay the same -- the
// instrument step of a retrieval iteration is then launches only, no upload (the weights kernel was 19 us of it).
// (the key held the buffer's ADDRESS; a call with more rays re-allocates the buffer -- the partial sums
// follow the table in it -- and the new block can come back at the old address with nothing in it.  The key is the
// buffer's generation now, and the device: the thread-local buffers follow a hipSetDevice())
struct LowresState {
  Stager s_bands, s_land; // the bands' centres / widths on their way up; the band spectra's pinned landing buffer
  DevBuf d_out;
  DevBuf d_weights;       // the bands' weight table [n_bands][n_pts] + point ranges, then the partial sums
  int64_t n_pts = -1, g_lo = 0;
  double w0 = 0, step = 0, n_sigma = 0;
  bool valid = false;
  bool instr = false;     // the table is the three tables of a call with the instrument derivatives (another layout)
  unsigned gen = 0;
  int dev = -1;
  std::vector<double> bands;
  bool ils = false;       // the table was made from a tabulated line shape: that binding's generation and shape
  unsigned ils_gen = 0;
  int ils_shapes = 0, ils_tab = 0;
  double ils_lo = 0, ils_hi = 0;
};
static thread_local LowresState t_lowres;

// The calling thread's instrument line shape (sr_set_ils): off -- the Gaussian over +-n_sigma widths, as the library always
// was -- or a table of knots.  tab [n_shapes][n_tab][2]: knot k and its slope per knot interval (the central difference
// (phi_(k+1) - phi_(k-1)) / 2 inside, the one-sided difference at the two ends: h times the slopes of the cubic Hermite
// interpolant), formed here once in fp64, as sr_lowres_weights_tab_kernel reads them.  gen: a new value with every
// binding, part of the weight table's key (the same bands under another shape are another table).
struct IlsState {
  bool on = false;
  int n_shapes = 0, n_tab = 0;
  double t_lo = 0, t_hi = 0;
  unsigned gen = 0;
  std::vector<double> tab;
};
static thread_local IlsState t_ils;
static void ils_slopes(const double *phi, int n_tab, double *knots_slopes) {
  for (int k = 0; k < n_tab; ++k) {
    knots_slopes[2 * k] = phi[k];
    knots_slopes[2 * k + 1] = k == 0 ? phi[1] - phi[0] : k == n_tab - 1 ? phi[k] - phi[k - 1] : (phi[k + 1] - phi[k - 1]) / 2.0;
  }
}
static int ils_check(const sr_ils_desc *ils) {
  if (!ils->phi || ils->n_shapes < 1 || ils->n_tab < 4) return SR_ERR_ARG;
  if (ils->n_tab > SR_MAX_ILS_TAB) return SR_ERR_LIMIT;
  if (!std::isfinite(ils->t_lo) || !std::isfinite(ils->t_hi) || !(ils->t_lo < ils->t_hi)) return SR_ERR_ARG;
  if ((size_t)ils->n_shapes > ((size_t)1 << 28) / (size_t)ils->n_tab) return SR_ERR_LIMIT;
  for (size_t k = 0; k < (size_t)ils->n_shapes * ils->n_tab; ++k)
    if (!std::isfinite(ils->phi[k])) return SR_ERR_ARG;
  return SR_OK;
}

// The instrument step's arguments (on their own for sr_retrieval_forward_dev, which checks before it touches its handle)
static int lowres_check(int n_rows, int64_t n_pts, int64_t g_lo, double w0, double step, const double *centers_nm,
                        const double *widths_nm, int n_bands, double n_sigma, int out_units) {
  if (!centers_nm || !widths_nm || n_rows <= 0 || n_pts < 2 || n_bands <= 0 || g_lo < 0) return SR_ERR_ARG;
  if (t_ils.on && t_ils.n_shapes != 1 && t_ils.n_shapes != n_bands) { // a table per band, and not this many bands
    g_err = "the bound line shape has " + std::to_string(t_ils.n_shapes) + " tables, the call " + std::to_string(n_bands) + " bands";
    return SR_ERR_ARG;
  }
  if (g_lo + n_pts > 2000000) return SR_ERR_LIMIT;
  if (!(step > 0.0) || !(w0 > 0.0) || !(n_sigma > 0.0) || out_units < 0 || out_units > 2) return SR_ERR_ARG;
  for (int b = 0; b < n_bands; ++b)
    if (!(widths_nm[b] > 0.0)) return SR_ERR_ARG;
  return SR_OK;
}
// Arguments checked, buffers for n_rows spectra in place, the weight table valid on `st` (its kernel launched there when
// the key changed: *fresh).  fused: partial sums per 64-point slot (launch_fold_dense with the scratch).  instr: the
// tables of the two instrument derivatives too (n_rows counts their rows); part of the key, the layouts differ.
// The one place that reads the thread's line shape (sr_set_ils): a table travels up with the bands, picks
// sr_lowres_weights_tab_kernel and joins the key with its generation and shape.
static int lowres_prepare(int n_rows, int64_t n_pts, int64_t g_lo, double w0, double step, const double *centers_nm,
                          const double *widths_nm, int n_bands, double n_sigma, int out_units, bool fused, hipStream_t st,
                          bool *fresh, bool instr = false) {
  int rc = lowres_check(n_rows, n_pts, g_lo, w0, step, centers_nm, widths_nm, n_bands, n_sigma, out_units);
  if (rc) return rc;
  LowresState &L = t_lowres;
  const size_t nb = (size_t)n_bands;
  int cur_dev = 0;
  HIPCHK(hipGetDevice(&cur_dev));
  if (L.dev != cur_dev) { // buffers of another device: start over on this one
    L.d_out.release();
    L.d_weights.release();
    L.valid = false;
    L.dev = cur_dev;
  }
  rc = L.d_out.ensure(sizeof(double) * nb * n_rows);
  if (rc) return rc;
  rc = L.d_weights.ensure(lowres_scratch_bytes((int)n_pts, n_bands, n_rows, fused, instr));
  if (rc) return rc;
  const IlsState &I = t_ils;
  const bool same_ils = L.ils == I.on && (!I.on || (L.ils_gen == I.gen && L.ils_shapes == I.n_shapes && L.ils_tab == I.n_tab &&
                                                    L.ils_lo == I.t_lo && L.ils_hi == I.t_hi));
  const bool same = L.valid && same_ils && L.instr == instr && L.gen == L.d_weights.gen && L.n_pts == n_pts && L.g_lo == g_lo && L.w0 == w0 && L.step == step &&
                    L.n_sigma == n_sigma && L.bands.size() == 2 * nb &&
                    std::memcmp(L.bands.data(), centers_nm, sizeof(double) * nb) == 0 &&
                    std::memcmp(L.bands.data() + nb, widths_nm, sizeof(double) * nb) == 0;
  *fresh = !same;
  if (same) return SR_OK;
  L.valid = false; // (until the launch below has been issued)
  const size_t n_up = 2 * nb + (I.on ? I.tab.size() : 0); // centres, widths, then the table
  rc = L.s_bands.prepare(sizeof(double) * n_up);
  if (rc) return rc;
  std::memcpy(L.s_bands.host<double>(), centers_nm, sizeof(double) * nb);
  std::memcpy(L.s_bands.host<double>() + nb, widths_nm, sizeof(double) * nb);
  if (I.on) std::memcpy(L.s_bands.host<double>() + 2 * nb, I.tab.data(), sizeof(double) * I.tab.size());
  rc = L.s_bands.push(sizeof(double) * n_up, st);
  if (rc) return rc;
  if (I.on)
    LAUNCHCHK(launch_lowres_weights_tab((int)n_pts, (int)g_lo, w0, step, L.s_bands.d.as<double>(), L.s_bands.d.as<double>() + nb,
                                        n_bands, L.s_bands.d.as<double>() + 2 * nb, I.n_shapes, I.n_tab, I.t_lo, I.t_hi,
                                        L.d_weights.p, st, instr));
  else
    LAUNCHCHK(launch_lowres_weights((int)n_pts, (int)g_lo, w0, step, L.s_bands.d.as<double>(), L.s_bands.d.as<double>() + nb, n_bands,
                                    n_sigma, L.d_weights.p, st, instr));
  L.ils = I.on; L.ils_gen = I.gen; L.ils_shapes = I.n_shapes; L.ils_tab = I.n_tab; L.ils_lo = I.t_lo; L.ils_hi = I.t_hi;
  L.instr = instr;
  L.n_pts = n_pts; L.g_lo = g_lo; L.w0 = w0; L.step = step; L.n_sigma = n_sigma;
  L.bands.assign(centers_nm, centers_nm + nb);
  L.bands.insert(L.bands.end(), widths_nm, widths_nm + nb);
  L.gen = L.d_weights.gen;
  L.valid = true; // (the callers synchronise `st` before they return: the table is complete before any later call)
  return SR_OK;
}

// d_out [n_rows][n_bands] to the host through a pinned buffer of the library's own (a copy into the caller's pageable
// memory is staged by the runtime); synchronises `st`
static int lowres_land(int n_rows, int n_bands, double *out_host, hipStream_t st) {
  LowresState &L = t_lowres;
  const size_t bytes = sizeof(double) * (size_t)n_bands * n_rows;
  const int rc = L.s_land.prepare(bytes);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(L.s_land.h, L.d_out.p, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::memcpy(out_host, L.s_land.h, bytes);
  return SR_OK;
}

// The band spectra of a ray batch and their derivatives on their way out (sr_retrieval_forward_dev,
// sr_limb_rays_state_bands_dev).  low: [n_rays + n_rays n_par][n_bands], the radiances' rows first, then row
// n_rays + r n_par + p; out: [n_pix or n_rays][1 + n_par][n_bands].  fov [n_pix][7] (see sr_retrieval_forward_dev): the
// closed-form field-of-view integral of every pixel's three rays, the operations of the mirror's fov_closed_form in its
// order; null: the rays themselves.
static void fov_rows(const double *low, int n_rays, int n_par, int n_bands, const double *fov, double *out) {
  const int n_row = 1 + n_par;
  // row of (ray r, quantity q): q = 0 the radiance, q = 1 + p the derivative to parameter p
  auto row = [&](int r, int q) { return low + (size_t)(q == 0 ? r : n_rays + r * n_par + (q - 1)) * n_bands; };
  if (!fov) {
    for (int r = 0; r < n_rays; ++r)
      for (int q = 0; q < n_row; ++q) std::memcpy(out + ((size_t)r * n_row + q) * n_bands, row(r, q), sizeof(double) * n_bands);
    return;
  }
  for (int px = 0; px < n_rays / 3; ++px) {
    const double *f = fov + 7 * px;
    const double delta = f[0], delta3 = f[1], two_dmax2 = f[2], edge = f[3], m2 = f[4], esse = f[5];
    const bool has_edge = f[6] != 0.0;
    for (int q = 0; q < n_row; ++q) {
      const double *s0 = row(3 * px, q), *s1 = row(3 * px + 1, q), *s2 = row(3 * px + 2, q);
      double *o = out + ((size_t)px * n_row + q) * n_bands;
      for (int b = 0; b < n_bands; ++b) { // (the operations of fov_closed_form, in its order)
        const double c = (s0[b] + s2[b] - 2.0 * s1[b]) / two_dmax2;
        double total = 2.0 * (s1[b] * delta + c * delta3 / 3.0);
        if (has_edge) total = total + s1[b] * edge + 2.0 * c * m2 / edge;
        o[b] = esse * total;
      }
    }
  }
}

// The radiance route of a batch without parameters keeps packed records: packed again from the columns, on `st`
static int los_repack(const sr_los *h, hipStream_t st) {
  if (h->n_par != 0 || h->F.n_rec <= 0) return 0;
  return launch_fold_fwd(h->F.plan, h->D.col, h->D.n_seg, h->F.n_rec, h->F.rec, nullptr, nullptr, 0, h->n_layers, h->opt.n_rays,
                         h->F.n_vis, limb_opts(&h->opt, h->D.n_seg), nullptr, st);
}

// the recursion of a resident LOS on `st`: launches only
static int limb_rays_los(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                         double *rad, hipStream_t st) {
  LosScope scope(h, st);
  const int rc0 = scope.enter();
  if (rc0) return rc0;
  sr_los_desc o = h->opt;
  o.g_lo = g_lo;
  if (h->F.n_rec > 0 && !limb_launch_is_small((int)n_pts, o.n_rays) && g_jac_layer_forward.load() == 0) {
    LAUNCHCHK(launch_fold_fwd(h->F.plan, h->D.col, h->D.n_seg, h->F.n_rec, h->F.rec, abs_c, emi_c, (int)n_pts, n_layers, o.n_rays,
                              h->F.n_vis, limb_opts(&o, h->D.n_seg), rad, st, /*pack=*/false));
    g_last_limb_route = 2;
    return scope.leave();
  }
  LAUNCHCHK(launch_limb(abs_c, emi_c, (int)n_pts, n_layers, o.n_rays, h->D.seg_off, h->D.seg_layer, h->D.col,
                        limb_opts(&o, h->D.n_seg), rad, st));
  g_last_limb_route = 1;
  return scope.leave();
}

// the launches of sr_limb_rays_jac_los_dev on `st`, inside the caller's LosScope
static int limb_jac_los(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo, double *rad,
                        double *jac, hipStream_t st) {
  sr_los_desc o = h->opt;
  o.g_lo = g_lo;
  if (h->n_par <= kFoldDensePar && h->F.n_rec > 0 && g_jac_layer_forward.load() == 0) {
    LAUNCHCHK(launch_fold_dense(h->F.plan, h->D.col, h->par_gas.data(), h->n_par, h->D.n_seg, h->F.n_rec, h->F.rec, abs_c, emi_c,
                                (int)n_pts, n_layers, o.n_rays, h->F.n_vis, limb_opts(&o, h->D.n_seg), rad, jac, st));
    return SR_OK;
  }
  LAUNCHCHK(launch_limb_jac(abs_c, emi_c, (int)n_pts, n_layers, o.n_rays, h->D.seg_off, h->D.seg_layer, h->D.col,
                            h->D.col + (size_t)o.n_gas * h->D.n_seg, h->D.par_gas, h->n_par, limb_opts(&o, h->D.n_seg), rad,
                            jac, st));
  return SR_OK;
}

extern "C" {

int sr_los_create_par(const sr_los_desc *los, int n_layers, int n_par, const int32_t *par_gas, const double *par_w,
                      sr_los **out) {
  if (!out || n_layers <= 0 || n_par < 0) return SR_ERR_ARG;
  *out = nullptr;
  LosShape shape;
  // (a batch made with parameters serves the entries of the folded and forward-sensitivity kernels only -- sr_limb_rays_jac_los_dev,
  // sr_retrieval_forward / _step / _loop_dev: refused here, they never see a handle of more than kFoldGasMax gases)
  int rc = check_los_par(los, n_layers, n_par, par_gas, par_w, &shape, n_par > 0 ? kFoldGasMax : kLimbGasMax);
  if (rc) return rc;
  sr_los *h = new sr_los();
  rc = stage_los(los, shape, n_par, par_gas, par_w, nullptr, &h->D, &h->s_los);
  if (!rc) rc = stage_fold(los, n_layers, nullptr, &h->F, &h->s_fold);
  if (!rc && n_par == 0 && h->F.n_rec > 0) { // (with parameters the records are packed per call: the columns change with the VMRs)
    LimbOpts o = limb_opts(los, h->D.n_seg);
    rc = launch_fold_fwd(h->F.plan, h->D.col, h->D.n_seg, h->F.n_rec, h->F.rec, nullptr, nullptr, 0, n_layers, los->n_rays,
                         h->F.n_vis, o, nullptr, nullptr) ? SR_ERR_HIP : SR_OK;
  }
  if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = SR_ERR_HIP; // (the null stream waited for the copy stream's work)
  if (rc) {
    h->s_los.release();
    h->s_fold.release();
    delete h;
    return rc;
  }
  h->opt = *los;
  h->opt.seg_off = h->opt.seg_layer = h->opt.pt_off = nullptr;
  h->opt.x = h->opt.nd = h->opt.vmr = h->opt.col_scale = nullptr;
  h->n_layers = n_layers;
  h->n_par = n_par;
  if (n_par > 0) h->par_gas.assign(par_gas, par_gas + n_par);
  (void)hipGetDevice(&h->dev);
  *out = h;
  return SR_OK;
}

int sr_los_create(const sr_los_desc *los, int n_layers, sr_los **out) {
  return sr_los_create_par(los, n_layers, 0, nullptr, nullptr, out);
}

int sr_los_destroy(sr_los *h) {
  if (!h) return SR_OK;
  h->s_los.release();
  h->s_fold.release();
  h->s_vmr.release();
  h->s_x.release();
  if (h->ev_last) (void)hipEventDestroy(h->ev_last);
  if (h->ev_k0) (void)hipEventDestroy(h->ev_k0);
  if (h->ev_k1) (void)hipEventDestroy(h->ev_k1);
  delete h;
  return SR_OK;
}

// New VMRs at the sample points of a resident batch (a retrieval iteration: paths, densities and parameter weights
// stay): one small copy and the column integration of the gases' profiles, on `stream`.
int sr_los_set_vmr(sr_los *h, const double *vmr, void *stream) {
  if (!h || !vmr) return SR_ERR_ARG;
  if (h->opt.los_order != 0) {
    g_err = "sr_los_set_vmr: batches in observer order re-list their sample points; build a new handle";
    return SR_ERR_UNSUPPORTED;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t bytes = sizeof(double) * (size_t)h->opt.n_gas * h->D.n_pt;
  LosScope scope(h, st);
  int rc = scope.enter();
  if (rc) return rc;
  rc = h->s_vmr.prepare(bytes); // (waits for the previous update's copy: the one pinned buffer is being refilled)
  if (rc) return rc;
  std::memcpy(h->s_vmr.host<char>(), vmr, bytes);
  // straight into the batch's profile table: [n_gas + n_par][n_pt], the gases first
  HIPCHK(hipMemcpyAsync(const_cast<double *>(h->D.prof), h->s_vmr.h, bytes, hipMemcpyHostToDevice, st));
  rc = h->s_vmr.mark(st);
  if (rc) return rc;
  LAUNCHCHK(launch_los_columns(h->D.nd, h->D.x, h->D.prof, h->D.scale, h->D.pt_off, h->D.n_seg, h->D.n_pt, h->opt.n_gas, h->D.col, st));
  LAUNCHCHK(los_repack(h, st));
  return scope.leave();
}

// The Curtis-Godson columns of a resident batch integrated again from its staged sample points (and the folded
// records repacked): two launches on `stream`, nothing copied.  For callers whose step is "columns + recursion" by
// definition (bench.py: the timed step keeps the column integration on the device, it only no longer re-stages a
// batch that has not changed).
int sr_los_refresh_columns(sr_los *h, void *stream) {
  if (!h) return SR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LosScope scope(h, st);
  const int rc0 = scope.enter();
  if (rc0) return rc0;
  LAUNCHCHK(launch_los_columns(h->D.nd, h->D.x, h->D.prof, h->D.scale, h->D.pt_off, h->D.n_seg, h->D.n_pt, h->D.n_prof, h->D.col, st));
  LAUNCHCHK(los_repack(h, st));
  return scope.leave();
}

// sr_limb_rays_jac_dev on a resident batch made with its column parameters (sr_los_create_par): launches only.
int sr_limb_rays_jac_los_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                             double *rad, double *jac, void *stream) {
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, rad && jac && h && n_layers == h->n_layers && h->n_par > 0);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LosScope scope(h, st);
  rc = scope.enter();
  if (rc) return rc;
  rc = limb_jac_los(abs_c, emi_c, n_layers, n_pts, h, g_lo, rad, jac, st);
  return rc ? rc : scope.leave();
}

// The forward model of ONE retrieval iteration on a resident batch made with its parameters, in one call: parameter
// vector -> VMRs of the retrieved gases at the sample points (sr_los_vmr_from_params_kernel) -> Curtis-Godson columns
// -> radiances and parameter Jacobians of every ray (one launch) -> instrument bands (sr_hires_to_lowres_shard_dev's
// kernels, its cached band weights) -> one copy to the host -> the closed-form field-of-view integral of every pixel
// (three rays each; spect_main_module.py:3342-3374 in the closed form of the mirror's fov_closed_form, geometry factors
// from the caller).  What spect_main_module.py:2736-2940 does per iteration between add_clim and chicalc.
//   buf: device scratch [n_rays (1 + n_par)][n_pts] (radiances' rows first)
//   fov: [n_pix][7] = delta, delta^3, 2 dmax^2, edge, m2, esse, has_edge (0 / 1) per pixel, n_pix = n_rays / 3; or null: no
//        field of view, `out` then holds the rays themselves
//   out: host [n_pix or n_rays][1 + n_par][n_bands]
int sr_retrieval_forward_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                             const double *x, double w0, double step, const double *centers_nm, const double *widths_nm,
                             int n_bands, double n_sigma, int out_units, const double *fov, double *buf, double *out,
                             void *stream) {
  if (!h || !x || !buf || !out || h->n_par <= 0 || n_bands <= 0) return SR_ERR_ARG;
  if (h->opt.init_mode == 1) return SR_ERR_ARG; // (initial radiances from the output buffer: `buf` is scratch here)
  const int n_rays = h->opt.n_rays, n_par = h->n_par, n_row = 1 + n_par;
  if (fov && n_rays % 3 != 0) return SR_ERR_ARG;
  // the tables, the grid and the bands too, before the handle's profiles and columns are rewritten
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, n_layers == h->n_layers);
  if (!rc) rc = lowres_check(n_rays * n_row, n_pts, g_lo, w0, step, centers_nm, widths_nm, n_bands, n_sigma, out_units);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LosScope scope(h, st);
  rc = scope.enter();
  if (rc) return rc;
  LAUNCHCHK(launch_los_vmr_from_params(const_cast<double *>(h->D.prof), h->opt.n_gas, n_par, h->D.n_pt, h->D.par_gas, x, st));
  LAUNCHCHK(launch_los_columns(h->D.nd, h->D.x, h->D.prof, h->D.scale, h->D.pt_off, h->D.n_seg, h->D.n_pt, h->opt.n_gas, h->D.col, st));
  static thread_local std::vector<double> low; // [n_rays + n_rays n_par][n_bands]
  low.resize((size_t)n_rays * n_row * n_bands);
  if (g_band_fusion.load() && n_par <= kFoldDensePar && h->F.n_rec > 0 && g_jac_layer_forward.load() == 0) {
    // the one-sweep kernel integrates the bands in its epilogue: no spectra are written (`buf` stays untouched)
    bool fresh = false;
    rc = lowres_prepare(n_rays * n_row, n_pts, g_lo, w0, step, centers_nm, widths_nm, n_bands, n_sigma, out_units, /*fused=*/true, st,
                        &fresh);
    if (rc) return rc;
    sr_los_desc o = h->opt;
    o.g_lo = g_lo;
    const bool timed = g_timing.load() == 2;
    if (timed) {
      if (!h->ev_k0) {
        HIPCHK(hipEventCreate(&h->ev_k0));
        HIPCHK(hipEventCreate(&h->ev_k1));
      }
      HIPCHK(hipEventRecord(h->ev_k0, st));
    }
    LAUNCHCHK(launch_fold_dense(h->F.plan, h->D.col, h->par_gas.data(), n_par, h->D.n_seg, h->F.n_rec, h->F.rec, abs_c, emi_c,
                                (int)n_pts, n_layers, n_rays, h->F.n_vis, limb_opts(&o, h->D.n_seg), buf, buf + (size_t)n_rays * n_pts,
                                st, t_lowres.d_weights.p, n_bands));
    if (timed) HIPCHK(hipEventRecord(h->ev_k1, st));
    h->k_timed = timed;
    rc = scope.leave();
    if (rc) return rc;
    // the sums go straight into the library's pinned landing buffer (16 KB over the bus from the kernel itself: no copy
    // command behind it)
    const size_t low_bytes = sizeof(double) * (size_t)n_rays * n_row * n_bands;
    rc = t_lowres.s_land.prepare(low_bytes);
    if (rc) return rc;
    LAUNCHCHK(launch_lowres_sum_blocks((int)n_pts, n_rays * n_row, n_bands, out_units, static_cast<double *>(t_lowres.s_land.h),
                                       t_lowres.d_weights.p, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(low.data(), t_lowres.s_land.h, low_bytes);
  } else {
    rc = limb_jac_los(abs_c, emi_c, n_layers, n_pts, h, g_lo, buf, buf + (size_t)n_rays * n_pts, st);
    if (!rc) rc = scope.leave();
    if (rc) return rc;
    rc = sr_hires_to_lowres_shard_dev(buf, n_rays * n_row, n_pts, g_lo, w0, step, centers_nm, widths_nm, n_bands, n_sigma, out_units,
                                      low.data(), stream);
    if (rc) return rc;
  }
  fov_rows(low.data(), n_rays, n_par, n_bands, fov, out);
  return SR_OK;
}

// n x n systems of the optimal-estimation step, host fp64: LU with partial pivoting (what numpy.linalg.solve / inv do
// through LAPACK's dgesv, unblocked).  a: [n][n] row-major, destroyed; b: [n][m] right-hand sides, overwritten with
// the solutions.  false: singular.
static bool lu_solve(std::vector<double> &a, int n, std::vector<double> &b, int m) {
  for (int k = 0; k < n; ++k) {
    int piv = k;
    for (int i = k + 1; i < n; ++i)
      if (std::fabs(a[(size_t)i * n + k]) > std::fabs(a[(size_t)piv * n + k])) piv = i;
    if (a[(size_t)piv * n + k] == 0.0) return false;
    if (piv != k) {
      for (int j = 0; j < n; ++j) std::swap(a[(size_t)k * n + j], a[(size_t)piv * n + j]);
      for (int j = 0; j < m; ++j) std::swap(b[(size_t)k * m + j], b[(size_t)piv * m + j]);
    }
    for (int i = k + 1; i < n; ++i) {
      const double f = a[(size_t)i * n + k] / a[(size_t)k * n + k];
      if (f == 0.0) continue;
      for (int j = k + 1; j < n; ++j) a[(size_t)i * n + j] -= f * a[(size_t)k * n + j];
      for (int j = 0; j < m; ++j) b[(size_t)i * m + j] -= f * b[(size_t)k * m + j];
    }
  }
  for (int k = n - 1; k >= 0; --k)
    for (int j = 0; j < m; ++j) {
      double v = b[(size_t)k * m + j];
      for (int i = k + 1; i < n; ++i) v -= a[(size_t)k * n + i] * b[(size_t)i * m + j];
      b[(size_t)k * m + j] = v / a[(size_t)k * n + k];
    }
  return true;
}

int sr_retrieval_step_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                          const double *x, double w0, double step, const double *centers_nm, const double *widths_nm,
                          int n_bands, double n_sigma, int out_units, const double *fov, double *buf, double *out,
                          const sr_oe_desc *oe, double *chi_sum, int32_t *n_used, double *dx, double *s_x, double *avk,
                          void *stream) {
  if (!h || !oe || !oe->obs || !oe->noise || !oe->sa_inv || !oe->x_apriori || !chi_sum || !n_used || !dx || !s_x || !avk)
    return SR_ERR_ARG;
  const int n_rays = h->opt.n_rays, n_par = h->n_par, n_row = 1 + n_par;
  if (n_rays % 3 != 0 || n_par <= 0 || n_par > 64) return SR_ERR_ARG;
  const int n_pix = n_rays / 3;
  if (oe->n_obs != n_pix * n_bands) return SR_ERR_ARG;
  // forward model: with a field of view straight into `out`; without one the centre ray of every three
  static thread_local std::vector<double> rays;
  double *fwd = out;
  if (!fov) {
    rays.resize((size_t)n_rays * n_row * n_bands);
    fwd = rays.data();
  }
  const int rc = sr_retrieval_forward_dev(abs_c, emi_c, n_layers, n_pts, h, g_lo, x, w0, step, centers_nm, widths_nm, n_bands,
                                          n_sigma, out_units, fov, buf, fwd, stream);
  if (rc) return rc;
  if (!fov)
    for (int px = 0; px < n_pix; ++px)
      std::memcpy(out + (size_t)px * n_row * n_bands, fwd + (size_t)(3 * px + 1) * n_row * n_bands, sizeof(double) * n_row * n_bands);
  // the used observations: K [n_used][n_par] (build_jacobian: pixel-major, band-minor), y - F, 1 / sigma^2
  const int n_obs = oe->n_obs;
  std::vector<double> K, resid, w;
  K.reserve((size_t)n_obs * n_par);
  resid.reserve(n_obs);
  w.reserve(n_obs);
  double chi = 0.0;
  for (int px = 0; px < n_pix; ++px)
    for (int b = 0; b < n_bands; ++b) {
      const int i = px * n_bands + b;
      if (oe->mask && !oe->mask[i]) continue;
      const double *rowp = out + (size_t)px * n_row * n_bands;
      const double d = oe->obs[i] - rowp[b];
      const double q = d / oe->noise[i];
      chi += q * q;                                                   // chicalc, :3400-3410
      resid.push_back(d);
      w.push_back(1.0 / (oe->noise[i] * oe->noise[i]));
      for (int p = 0; p < n_par; ++p) K.push_back(rowp[(size_t)(1 + p) * n_bands + b]);
    }
  const int nu = (int)resid.size();
  *chi_sum = chi;
  *n_used = nu;
  // inversion_algebra (:3433-3469)
  const size_t np2 = (size_t)n_par * n_par;
  std::vector<double> G(np2, 0.0), rhs((size_t)n_par, 0.0);
  for (int i = 0; i < nu; ++i) {
    const double *k = K.data() + (size_t)i * n_par;
    for (int p = 0; p < n_par; ++p) {
      const double kw = k[p] * w[i];                                   // KtSy[p][i]
      rhs[p] += kw * resid[i];
      for (int q = 0; q < n_par; ++q) G[(size_t)p * n_par + q] += kw * k[q];
    }
  }
  std::vector<double> S_inv(np2), A(np2), I(np2, 0.0);
  for (size_t e = 0; e < np2; ++e) S_inv[e] = G[e] + oe->sa_inv[e];
  for (int p = 0; p < n_par; ++p) {
    double acc = 0.0;
    for (int q = 0; q < n_par; ++q) acc += oe->sa_inv[(size_t)p * n_par + q] * (oe->x_apriori[q] - x[q]);
    rhs[p] += acc;
    I[(size_t)p * n_par + p] = 1.0;
  }
  A = S_inv;
  if (!lu_solve(A, n_par, I, n_par)) return SR_ERR_TABLE;              // S_x = inv(S_inv)
  std::memcpy(s_x, I.data(), sizeof(double) * np2);
  for (int p = 0; p < n_par; ++p)
    for (int q = 0; q < n_par; ++q) {
      double acc = 0.0;
      for (int r = 0; r < n_par; ++r) acc += I[(size_t)p * n_par + r] * G[(size_t)r * n_par + q];
      avk[(size_t)p * n_par + q] = acc;                                // AVK = S_x G
    }
  A = S_inv;
  for (int p = 0; p < n_par; ++p) A[(size_t)p * n_par + p] += oe->lambda_lm * S_inv[(size_t)p * n_par + p];
  if (!lu_solve(A, n_par, rhs, 1)) return SR_ERR_TABLE;
  std::memcpy(dx, rhs.data(), sizeof(double) * (size_t)n_par);
  return SR_OK;
}

int sr_los_last_kernel_ms(sr_los *h, float *ms) {
  if (!h || !ms || !h->k_timed) return SR_ERR_ARG;
  HIPCHK(hipEventSynchronize(h->ev_k1));
  HIPCHK(hipEventElapsedTime(ms, h->ev_k0, h->ev_k1));
  return SR_OK;
}

// The retrieval loop itself (spect_main_module.py:2725-2987 with fixed coefficient spectra): sr_retrieval_step_dev per
// iteration, reduced chi square (:2949), stopping rule (:2960-2973), the update with the positivity rule (:616-624).
int sr_retrieval_loop_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                          const double *x0, double w0, double step, const double *centers_nm, const double *widths_nm,
                          int n_bands, double n_sigma, int out_units, const double *fov, double *buf, double *out,
                          const sr_oe_desc *oe, const sr_loop_desc *lp, double *chi_hist, double *x_hist, int32_t *n_it,
                          int32_t *stop, double *s_x, double *avk, void *stream) {
  if (!h || !x0 || !oe || !lp || !lp->positive || !chi_hist || !x_hist || !n_it || !stop || !s_x || !avk || lp->max_it < 0)
    return SR_ERR_ARG;
  const int n_par = h->n_par;
  if (n_par <= 0 || n_par > 64) return SR_ERR_ARG;
  const size_t np2 = (size_t)n_par * n_par;
  std::vector<double> x(x0, x0 + n_par), dx((size_t)n_par), sx(np2), av(np2);
  std::memcpy(x_hist, x.data(), sizeof(double) * (size_t)n_par);
  *n_it = 0;
  *stop = 0;
  double chi_old = 0.0;
  for (int it = 0; it < lp->max_it; ++it) {
    double chi_sum = 0.0;
    int32_t nu = 0;
    const int rc = sr_retrieval_step_dev(abs_c, emi_c, n_layers, n_pts, h, g_lo, x.data(), w0, step, centers_nm, widths_nm,
                                         n_bands, n_sigma, out_units, fov, buf, out, oe, &chi_sum, &nu, dx.data(), sx.data(),
                                         av.data(), stream);
    if (rc) return rc;
    const double chi = chi_sum / (double)(nu - lp->n_dof_par);
    chi_hist[it] = chi;
    *n_it = it + 1;
    if (it > 0) {
      if (std::fabs(chi - chi_old) / chi_old < lp->chi_threshold) { *stop = 1; break; }
      if (chi > chi_old) { *stop = 2; break; }
    }
    chi_old = chi;
    for (int p = 0; p < n_par; ++p) {
      double d = dx[p];
      if (lp->positive[p]) {
        if (!(x[p] > 0.0)) { // (the reference would halve for ever)
          g_err = "sr_retrieval_loop_dev: a positive-constrained parameter is not positive";
          return SR_ERR_ARG;
        }
        while (x[p] + d <= 0.0) d /= 2;
      }
      x[p] = x[p] + d;
    }
    std::memcpy(s_x, sx.data(), sizeof(double) * np2);
    std::memcpy(avk, av.data(), sizeof(double) * np2);
    std::memcpy(x_hist + (size_t)(it + 1) * n_par, x.data(), sizeof(double) * (size_t)n_par);
  }
  return SR_OK;
}

int sr_limb_rays_los_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                         double *rad, void *stream) {
  // (a batch made with parameters keeps no packed radiance records: sr_limb_rays_jac_los_dev)
  const int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, rad && h && n_layers == h->n_layers && h->n_par == 0);
  if (rc) return rc;
  return limb_rays_los(abs_c, emi_c, n_layers, n_pts, h, g_lo, rad, static_cast<hipStream_t>(stream));
}

int sr_limb_step_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *abs_out, double *emi_out,
                     sr_los *h, double *rad, void *stream) {
  if (!h || !rad || !atm || h->opt.n_gas != 1 || h->n_par != 0 || atm->n_layers != h->n_layers) return SR_ERR_ARG;
  const int rc = coef_op(ls, atm, g_lo, g_hi, abs_out, emi_out, stream, WeightMode{kWeightFolded, 0});
  if (rc) return rc;
  return limb_rays_los(abs_out, emi_out, atm->n_layers, g_hi - g_lo, h, g_lo, rad, static_cast<hipStream_t>(stream));
}

int sr_limb_rays_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, const sr_los_desc *los,
                     double *rad, void *stream) {
  LosShape shape;
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, rad != nullptr);
  if (!rc) rc = check_los(los, n_layers, &shape, kLimbGasMax);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LosDev D;
  rc = stage_los(los, shape, 0, nullptr, nullptr, st, &D);
  if (rc) return rc;
  // ray batches of a 1-D atmosphere: the folded sweep (a shell's loads and, the path being symmetric, its attenuation
  // once for the ray's two segments); small launches keep the split kernel, whose time is a chain's latency
  if (!limb_launch_is_small((int)n_pts, los->n_rays) && g_jac_layer_forward.load() == 0) {
    FoldStage F;
    rc = stage_fold(los, n_layers, st, &F);
    if (rc) return rc;
    if (F.n_rec > 0) {
      LAUNCHCHK(launch_fold_fwd(F.plan, D.col, D.n_seg, F.n_rec, F.rec, abs_c, emi_c, (int)n_pts, n_layers, los->n_rays, F.n_vis,
                                limb_opts(los, D.n_seg), rad, st));
      g_last_limb_route = 2;
      return mark_both(*F.slot, *D.slot, st);
    }
  }
  LAUNCHCHK(launch_limb(abs_c, emi_c, (int)n_pts, n_layers, los->n_rays, D.seg_off, D.seg_layer, D.col,
                        limb_opts(los, D.n_seg), rad, st));
  g_last_limb_route = 1;
  return D.slot->mark(st);
}

} // extern "C"

namespace {

// Radiances (rad may be NULL) + per-layer Jacobian (dabs / demi / jac_layer may be NULL) + column-parameter Jacobian
// (n_par may be 0) in one pass.  *done = 0 when the plan does not fit the kernel (nothing launched).  The callers have
// checked everything: the LOS and its parameters (check_los_par: `shape`), seg_jrow's range, rad against init_mode 1.
int limb_adjoint(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_layers,
                 int64_t n_pts, const sr_los_desc *los, const LosShape &shape, const int32_t *seg_jrow, int n_jrows, int n_par,
                 const int32_t *par_gas, const double *par_w, double *rad, double *jac_layer, double *jac_par,
                 hipStream_t st, int *done) {
  *done = 0;
  const int n_seg = shape.n_seg;
  if (!seg_jrow) n_jrows = n_layers;
  AdjPlan plan;
  if (!build_adj_plan(los, n_layers, seg_jrow, n_jrows, n_par, par_gas, par_w, jac_layer != nullptr, shape.n_pt, &plan)) return SR_OK;
  LosDev D;
  int rc = stage_los(los, shape, n_par, par_gas, par_w, st, &D);
  if (rc) return rc;
  // The route (sr_set_jac_layer_mode).  Rays that walk the shells down to a turning shell and up again (fold_sides) take
  // the folded kernel by default (mode 0; 3-D paths with their shells = Jacobian rows, a coefficient row per LOS step)
  // or, in mode 3 and when they share their coefficient rows, the layer-synchronous one.  Anything else -- an unordered
  // LOS, a folded plan that does not fit, modes 1 and 2 -- keeps one ray per thread in path order.
  std::vector<int> sched, fplan;
  int n_visits = 0, n_fvis = 0;
  const int nr = los->n_rays;
  const int jmode = g_jac_layer_forward.load();
  const bool two_rows = seg_jrow != nullptr;
  const int n_sh = two_rows ? n_jrows : n_layers; // shells
  if (jmode == 0 || (jmode == 3 && nr >= 2 && !two_rows)) {
    std::vector<int> far, near;
    int l_min = n_sh, l_max = -1;
    if (fold_sides(los, n_sh, seg_jrow, &far, &near, &l_min, &l_max)) {
      if (jmode == 0) {
        const std::vector<int> shells = fold_shells(far, near, nr, n_sh, l_min, l_max);
        if (build_fold_plan(plan, far, near, shells, nr, n_sh, two_rows, n_par, par_gas, &fplan)) n_fvis = (int)shells.size();
      } else {
        build_sync_schedule(far, near, nr, n_layers, l_min, l_max, &sched, &n_visits);
      }
    }
  }
  const int n_frec = nr * n_fvis;
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const auto p_plan = pk.copy(plan.seg.data(), plan.seg.size()), p_zo = pk.copy(plan.zero_off.data(), plan.zero_off.size());
  const auto p_zr = pk.copy(plan.zero_row.data(), plan.zero_row.size(), 1), p_sc = pk.copy(sched.data(), sched.size(), 1);
  const auto p_fp = pk.copy(fplan.data(), fplan.size(), 1);
  pk.tail(std::max(adj_prog_bytes(n_seg), fold_rec_bytes(n_frec))); // the packed records of the kernel that runs
  rc = pk.stage(st);
  if (rc) return rc;
  if (n_fvis > 0) {
    FoldRec *frec = pk.dev_tail<FoldRec>();
    LAUNCHCHK(launch_fold_pack(pk.dev(p_fp), D.col, los->n_gas, n_seg, n_frec, frec, st));
    LAUNCHCHK(launch_limb_adjoint_fold(abs_c, emi_c, dabs, demi, (int)n_pts, n_layers, n_jrows, two_rows ? 1 : 0, nr, frec,
                                       pk.dev(p_zo), pk.dev(p_zr), n_par, limb_opts(los, D.n_seg), n_fvis, rad, jac_layer,
                                       jac_par, st));
  } else {
    SegProg *prog = pk.dev_tail<SegProg>();
    LAUNCHCHK(launch_adj_pack(pk.dev(p_plan), D.col, los->n_gas, n_seg, prog, st));
    if (n_visits > 0)
      LAUNCHCHK(launch_limb_adjoint_sync(abs_c, emi_c, dabs, demi, (int)n_pts, n_layers, n_jrows, nr, prog, pk.dev(p_zo),
                                         pk.dev(p_zr), n_par, limb_opts(los, D.n_seg), pk.dev(p_sc), n_visits, rad, jac_layer,
                                         jac_par, st));
    else
      LAUNCHCHK(launch_limb_adjoint(abs_c, emi_c, dabs, demi, (int)n_pts, n_layers, n_jrows, los->n_rays, D.seg_off, prog,
                                    pk.dev(p_zo), pk.dev(p_zr), n_par, limb_opts(los, D.n_seg), rad, jac_layer, jac_par, st));
  }
  *done = 1;
  return mark_both(pk.slot(), *D.slot, st);
}

} // namespace

extern "C" {

int sr_limb_rays_jacobians_dev(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                               int n_layers, int64_t n_pts, const sr_los_desc *los, const int32_t *seg_jac_row,
                               int n_jac_rows, int n_par, const int32_t *par_gas, const double *par_w, double *rad,
                               double *jac_layer, double *jac_par, void *stream) {
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, n_par >= 0 && !(seg_jac_row && n_jac_rows <= 0));
  if (rc) return rc;
  const bool want_layer = jac_layer != nullptr, want_par = n_par > 0;
  if (want_layer != (dabs != nullptr && demi != nullptr) || (want_par && (!jac_par || !par_gas || !par_w))) return SR_ERR_ARG;
  if ((!want_layer && !want_par) || !los) return SR_ERR_ARG;
  if (!rad && los->init_mode == 1) { // the initial intensity would be read from rad (a NULL read on the device)
    g_err = "sr_limb_rays_jacobians_dev: init_mode 1 reads the initial intensity from rad, which is NULL";
    return SR_ERR_ARG;
  }
  if (want_layer) rc = refuse_init_mode_1(los, "sr_limb_rays_jacobians_dev (per-layer Jacobians)", SR_ERR_UNSUPPORTED);
  if (rc) return rc;
  for (int p = 0; p < n_par; ++p)
    if (par_gas[p] < 0 || par_gas[p] >= los->n_gas) return SR_ERR_ARG;
  const bool one_pass = g_jac_layer_forward.load() != 1;
  const auto needs_one_pass = [] {
    g_err = "sr_limb_rays_jacobians_dev: Jacobian rows other than the coefficient rows need the one-pass kernel "
            "(sr_set_jac_layer_mode(0) and at most four column parameters per segment)";
    return SR_ERR_UNSUPPORTED;
  };
  if (!one_pass && seg_jac_row && want_layer) return needs_one_pass();
  LosShape shape;
  rc = check_los(los, n_layers, &shape);
  if (rc) return rc;
  if (seg_jac_row && one_pass)
    for (int q = 0; q < shape.n_seg; ++q)
      if (seg_jac_row[q] < 0 || seg_jac_row[q] >= n_jac_rows) return SR_ERR_ARG; // would write out of the Jacobian
  hipStream_t st = static_cast<hipStream_t>(stream);
  int done = 0;
  if (one_pass) {
    rc = limb_adjoint(abs_c, emi_c, dabs, demi, n_layers, n_pts, los, shape, seg_jac_row, n_jac_rows, n_par, par_gas, par_w, rad,
                      jac_layer, jac_par, st, &done);
    if (rc || done) return rc;
  }
  // forward-sensitivity kernels, one call per kind (a segment touching more than four parameters, or asked for)
  if (seg_jac_row && want_layer) return needs_one_pass();
  if (want_par) {
    double *rad_out = rad;
    static thread_local DevBuf scratch_rad; // the forward kernel writes the radiances too: somewhere, if not wanted
    if (!rad_out) {
      const int rc0 = scratch_rad.ensure(sizeof(double) * (size_t)los->n_rays * (size_t)n_pts);
      if (rc0) return rc0;
      rad_out = scratch_rad.as<double>();
    }
    rc = sr_limb_rays_jac_dev(abs_c, emi_c, n_layers, n_pts, los, n_par, par_gas, par_w, rad_out, jac_par, stream);
    if (rc) return rc;
  }
  if (want_layer) {
    rc = sr_limb_rays_jac_layer_dev(abs_c, emi_c, dabs, demi, n_layers, n_pts, los, jac_layer, stream);
    if (rc) return rc;
    if (rad && !want_par) return sr_limb_rays_dev(abs_c, emi_c, n_layers, n_pts, los, rad, stream);
  }
  return SR_OK;
}

int sr_limb_rays_jac_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                         const sr_los_desc *los, int n_par, const int32_t *par_gas, const double *par_w, double *rad,
                         double *jac, void *stream) {
  LosShape shape;
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, rad && jac && n_par > 0);
  if (!rc) rc = check_los_par(los, n_layers, n_par, par_gas, par_w, &shape);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // many parameters: one pass per ray (the forward kernel repeats the recursion per 16 parameters); rad0 given
  // (init_mode 1) is read by both kernels before they write
  if (n_par > 8 && g_jac_layer_forward.load() != 1) {
    int done = 0;
    rc = limb_adjoint(abs_c, emi_c, nullptr, nullptr, n_layers, n_pts, los, shape, nullptr, 0, n_par, par_gas, par_w, rad, nullptr,
                      jac, st, &done);
    if (rc || done) return rc;
  }
  LosDev D;
  rc = stage_los(los, shape, n_par, par_gas, par_w, st, &D);
  if (rc) return rc;
  // Few parameters, 1-D limb / slant / nadir rays: the folded recursion with an accumulator per parameter
  // (sr_limb_fold_sens_lds_kernel) instead of the path-order forward sensitivities (which repeat the recursion per four parameters)
  if (n_par <= kFoldDensePar && g_jac_layer_forward.load() == 0) {
    FoldStage F;
    rc = stage_fold(los, n_layers, st, &F);
    if (rc) return rc;
    if (F.n_rec > 0) {
      LAUNCHCHK(launch_fold_dense(F.plan, D.col, par_gas, n_par, D.n_seg, F.n_rec, F.rec, abs_c, emi_c, (int)n_pts, n_layers,
                                  los->n_rays, F.n_vis, limb_opts(los, D.n_seg), rad, jac, st));
      return mark_both(*F.slot, *D.slot, st);
    }
  }
  LAUNCHCHK(launch_limb_jac(abs_c, emi_c, (int)n_pts, n_layers, los->n_rays, D.seg_off, D.seg_layer, D.col,
                            D.col + (size_t)los->n_gas * D.n_seg, D.par_gas, n_par, limb_opts(los, D.n_seg), rad, jac,
                            st));
  return D.slot->mark(st);
}

int sr_limb_rays_jac_layer_dev(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                               int n_layers, int64_t n_pts, const sr_los_desc *los, double *jac, void *stream) {
  LosShape shape;
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, dabs && demi && jac);
  if (!rc && los) rc = refuse_init_mode_1(los, "sr_limb_rays_jac_layer_dev", SR_ERR_UNSUPPORTED);
  if (!rc) rc = check_los(los, n_layers, &shape);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (g_jac_layer_forward.load() != 1 && n_layers > 8) {
    int done = 0;
    rc = limb_adjoint(abs_c, emi_c, dabs, demi, n_layers, n_pts, los, shape, nullptr, 0, 0, nullptr, nullptr, nullptr, jac, nullptr,
                      st, &done);
    if (rc || done) return rc;
  }
  LosDev D;
  rc = stage_los(los, shape, 0, nullptr, nullptr, st, &D);
  if (rc) return rc;
  LAUNCHCHK(launch_limb_jac_layer(abs_c, emi_c, dabs, demi, (int)n_pts, n_layers, los->n_rays, D.seg_off, D.seg_layer,
                                  D.col, limb_opts(los, D.n_seg), jac, st));
  return D.slot->mark(st);
}

// What the entries below do once their arguments are checked: plan, stage, launch, mark.  First the record they fill, a
// mixed-state call as its entry receives it, in blocks of what belongs together.
struct StateBatch { // the coefficient tables and the rays
  const double *abs_c, *emi_c;
  int n_layers;
  int64_t n_pts;
  const sr_los_desc *los;
};
struct StateCols { // column parameters, staged with the batch
  int n_col;
  const int32_t *par_gas;
  const double *par_w;
};
// level parameters: the level-factored gases come as a list -- the one-gas entries hand in their one (one_level_gas) --
// and par_lgas [n_lev] names a level parameter's level gas (null with one: all 0)
struct StateLevels {
  int n_lgas;
  const sr_level_gas *lgas;
  int n_lev;
  const int32_t *par_lgas, *par_level;
  const double *par_c;
};
struct StateRows { // row parameters, which act through dabs / demi
  const double *dabs_c, *demi_c;
  int n_row;
  const double *par_t;
};
// the instrument's bands instead of spectra; instr: with the two instrument rows behind the parameters'
struct StateBands {
  const double *centers_nm, *widths_nm;
  int n_bands;
  double n_sigma;
  int out_units;
  const double *fov;
  double *out;
  bool instr;
};
struct StateCall {
  const char *entry; // the name its messages carry
  StateBatch b;
  StateCols col;
  StateLevels lev;
  StateRows row;
  void *stream;
  // cols: the kernel instances with column slots (the state call, with n_col == 0 too); without them n_col is 0 and
  // neither blk nor dcol exists
  bool cols = false;
  double *rad = nullptr, *jac = nullptr; // the spectra, or
  const StateBands *bands = nullptr;     // the bands block
  // the pointing derivative: n_gas hidden column slots behind the caller's, their rows behind the state's (cols is set)
  const sr_los_path *path = nullptr;
};
static sr_level_gas one_level_gas(int gas, const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row) {
  sr_level_gas g;
  g.gas = gas; g.n_levels = n_levels; g.n_tab_rows = n_tab_rows; g.tab = tab; g.coef_row = coef_row;
  return g;
}

// n_row > 0: the instances with row slots, which read dabs / demi.  band_scratch (a call with a bands block): the
// instrument step's scratch with its weight table in place; the instances with the band epilogue then leave their partial
// sums there, rad and jac are not used.  With bands->instr it is the scratch of a call with the instrument derivatives,
// the INSTR instances; then there may be no parameter at all.
static int limb_jac_state(const StateCall &c, const LosShape &shape, const void *band_scratch, hipStream_t st) {
  const StateBatch &b = c.b;
  const int n_layers = b.n_layers, n_col = c.col.n_col, n_lev = c.lev.n_lev, n_row = c.row.n_row, n_lgas = c.lev.n_lgas;
  const sr_level_gas *lgas = c.lev.lgas;
  const bool several = n_lgas > 1;
  const int n_hid = c.path ? b.los->n_gas : 0, gas_bits = state_gas_bits(b.los->n_gas);
  // the dense plan, or (sr_set_state_ray_blocks) every ray's own blocks, whose tables take the dense plan's places
  const bool per_ray = g_state_ray_blocks.load() != 0;
  LevelJacPlan P{};
  RayJacPlan R{};
  if (per_ray) {
    R = ray_jac_plan(b.los, n_col, c.col.par_gas, c.col.par_w, n_lev, c.lev.par_level, c.lev.par_c, n_layers, n_row, c.row.par_t,
                     several ? c.lev.par_lgas : nullptr, n_hid, gas_bits);
    P.n_blocks = R.n_blocks;
    P.blk.swap(R.blk), P.ent_off.swap(R.ent_off), P.slot_par.swap(R.slot_par), P.ent.swap(R.ent);
  } else {
    P = level_jac_plan(n_col, c.col.par_gas, n_lev, c.lev.par_level, c.lev.par_c, n_layers, n_row, c.row.par_t,
                       several ? c.lev.par_lgas : nullptr, n_hid, gas_bits);
  }
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const auto p_ent = pk.copy(P.ent.data(), P.ent.size(), 1); // (no entries: a valid pointer all the same)
  const auto p_rboff = pk.copy(R.ray_blk_off.data(), R.ray_blk_off.size()), p_crow = pk.copy(R.col_row.data(), R.col_row.size());
  const int32_t *coef_row = lgas[0].coef_row;
  std::vector<int32_t> rows_all; // several level gases: their row maps one behind the other, [n_lgas][n_layers]
  if (several && n_lev > 0) {
    rows_all.reserve((size_t)n_lgas * n_layers);
    for (int k = 0; k < n_lgas; ++k) rows_all.insert(rows_all.end(), lgas[k].coef_row, lgas[k].coef_row + n_layers);
    coef_row = rows_all.data();
  }
  const size_t n_rowmap = (size_t)n_lgas * n_layers;
  const auto p_row = n_lev > 0 ? pk.copy(coef_row, n_rowmap) : pk.zeros<int32_t>(n_rowmap);
  const auto p_off = pk.copy(P.ent_off.data(), P.ent_off.size()), p_slot = pk.copy(P.slot_par.data(), P.slot_par.size());
  const auto p_blk = pk.copy(P.blk.data(), P.blk.size());
  int rc = pk.stage(st);
  if (rc) return rc;
  LosDev D;
  rc = stage_los(b.los, shape, n_col, c.col.par_gas, c.col.par_w, st, &D, nullptr, c.path);
  if (rc) return rc;
  LevelGasTabs lg{};
  for (int k = 0; several && k < n_lgas; ++k) {
    lg.tab[k] = lgas[k].tab;
    lg.n_tab_rows[k] = lgas[k].n_tab_rows;
    lg.gas[k] = lgas[k].gas;
  }
  StateLaunch L{};
  L.abs_c = b.abs_c, L.emi_c = b.emi_c;
  L.n_pts = (int)b.n_pts, L.n_layers = n_layers, L.n_rays = b.los->n_rays;
  L.seg_off = D.seg_off, L.seg_layer = D.seg_layer;
  L.col = D.col, L.dcol = c.cols ? D.col + (size_t)b.los->n_gas * D.n_seg : nullptr;
  L.o = limb_opts(b.los, D.n_seg);
  L.gas = lgas[0].gas, L.tab = lgas[0].tab, L.n_tab_rows = lgas[0].n_tab_rows;
  L.lgas = several ? &lg : nullptr;
  L.coef_row = pk.dev(p_row);
  L.n_blocks = P.n_blocks, L.blk = c.cols ? pk.dev(p_blk) : nullptr;
  L.ent_off = pk.dev(p_off), L.ent = pk.dev(p_ent), L.slot_par = pk.dev(p_slot);
  L.n_par = n_col + n_lev + n_row + n_hid;
  if (n_row > 0) L.dabs = c.row.dabs_c, L.demi = c.row.demi_c;
  L.rad = c.rad, L.jac = c.jac;
  if (c.bands) L.lowres_scratch = band_scratch, L.n_bands = c.bands->n_bands, L.instr = c.bands->instr;
  if (per_ray) L.ray_blk_off = pk.dev(p_rboff), L.col_row = pk.dev(p_crow), L.np = R.np;
  g_last_state_route = per_ray ? 2 : 1;
  g_last_state_walks = per_ray ? (int64_t)R.ray_blk_off.back() : (int64_t)L.n_rays * P.n_blocks;
  LAUNCHCHK(launch_limb_jac_state(L, st));
  if (n_hid && !c.bands) LAUNCHCHK(launch_jac_rows_sum(c.jac, L.n_rays, L.n_par - n_hid, n_hid, L.n_pts, st));
  return mark_both(pk.slot(), *D.slot, st);
}

// The arguments of the mixed-state calls (sr_limb_rays_jac_level_dev, sr_limb_rays_jac_state_dev, _state_rows_dev,
// sr_limb_rays_state_bands_dev and their forms for several level gases), all of them before the first copy or launch
// (the LOS too: stage_los would only find out after the call's own staging).  The caller's outputs must be there: jac,
// or out and the bands.  Any kind of parameter may be empty, not all (but for the calls with the instrument rows, which
// have something to return without a parameter); a kind that is empty needs none of its arrays.  With one level gas the
// checks and their order are what they always were.
static int check_state_call(const StateCall &c, LosShape *shape) {
  const StateBatch &b = c.b;
  const int n_col = c.col.n_col, n_lev = c.lev.n_lev, n_row = c.row.n_row, n_lgas = c.lev.n_lgas;
  const sr_level_gas *lgas = c.lev.lgas;
  const int32_t *par_lgas = c.lev.par_lgas, *par_level = c.lev.par_level;
  const bool out_ok = c.bands ? c.bands->out && c.bands->centers_nm && c.bands->widths_nm && c.bands->n_bands > 0 : c.jac != nullptr;
  const bool may_be_empty = (c.bands && c.bands->instr) || c.path;
  const bool list_ok = lgas && n_lgas >= 1 && n_lgas <= kLevelGasMax;
  bool lev_ok = n_lev == 0 || (list_ok && par_level && c.lev.par_c && (n_lgas == 1 || par_lgas));
  for (int k = 0; list_ok && n_lev > 0 && k < n_lgas; ++k)
    lev_ok = lev_ok && lgas[k].tab && lgas[k].coef_row && lgas[k].n_levels > 0 && lgas[k].n_tab_rows > 0;
  const bool row_ok = n_row == 0 || (c.row.dabs_c && c.row.demi_c && c.row.par_t);
  const bool counts_ok = n_col >= 0 && n_lev >= 0 && n_row >= 0 && (int64_t)n_col + n_lev + n_row >= (may_be_empty ? 0 : 1);
  int rc = check_limb_call(b.abs_c, b.emi_c, b.n_layers, b.n_pts, out_ok && counts_ok && list_ok && lev_ok && row_ok);
  if (!rc) rc = check_los_par(b.los, b.n_layers, n_col, c.col.par_gas, c.col.par_w, shape, kLimbGasMax);
  if (rc) return rc;
  if (n_lgas > b.los->n_gas) return SR_ERR_ARG;
  for (int k = 0; k < n_lgas; ++k) {
    if (lgas[k].gas < 0 || lgas[k].gas >= b.los->n_gas) return SR_ERR_ARG;
    for (int i = 0; i < k; ++i)
      if (lgas[i].gas == lgas[k].gas) return SR_ERR_ARG; // one gas of the batch, one set of tables
  }
  if ((rc = refuse_init_mode_1(b.los, c.entry, SR_ERR_ARG))) return rc;
  for (int k = 0; n_lev > 0 && k < n_lgas; ++k)
    if (!coef_rows_in_range(lgas[k].coef_row, b.n_layers, lgas[k].n_tab_rows)) return SR_ERR_ARG;
  for (int p = 0; p < n_lev; ++p) {
    const int k = par_lgas ? par_lgas[p] : 0;
    if (k < 0 || k >= n_lgas) return SR_ERR_ARG;
    if (par_level[p] < 0 || par_level[p] >= lgas[k].n_levels) return SR_ERR_ARG;
  }
  if ((int64_t)n_col + n_lev + n_row + (c.path ? b.los->n_gas : 0) > INT_MAX) return SR_ERR_LIMIT;
  if (c.path && b.los->los_order != 0) {
    g_err = std::string(c.entry) + ": the pointing derivative needs the batch in photon order (observer order re-lists the sample points)";
    return SR_ERR_UNSUPPORTED;
  }
  if (n_lgas > 1) // (an entry's word holds the level below kLevelEntGasShift)
    for (int k = 0; n_lev > 0 && k < n_lgas; ++k)
      if (lgas[k].n_levels > kLevelEntLevelMask + 1) return SR_ERR_LIMIT;
  return SR_OK;
}

// The calls that return spectra: checked, then run.
static int limb_state_spectra(const StateCall &c) {
  LosShape shape;
  const int rc = check_state_call(c, &shape);
  return rc ? rc : limb_jac_state(c, shape, nullptr, static_cast<hipStream_t>(c.stream));
}
// ... of one level gas with a row block.  Nothing of the third kind: the state call, checks and all; else, without
// column parameters, the instances without column code (fewer registers, the same arithmetic).
static int limb_state_rows(StateCall &c) {
  c.cols = c.col.n_col > 0 || c.path;
  if (c.row.n_row == 0) {
    c.entry = "sr_limb_rays_jac_state_dev";
    c.row = StateRows{};
    c.cols = true;
  }
  return limb_state_spectra(c);
}

// The mixed-state Jacobian on the instrument's bands: the state call's plan and checks, the instrument step's cached
// weight table (lowres_prepare, fused), the recursion kernel's band epilogue, the partial sums added straight into the
// pinned landing buffer, the field of view on the host.  One body for one level gas (the one-gas instances) and for
// several.
static int limb_state_bands(StateCall &c) {
  const StateBands &B = *c.bands;
  const sr_los_desc *los = c.b.los;
  const int64_t n_pts = c.b.n_pts;
  c.cols = c.col.n_col > 0 || c.path;
  LosShape shape;
  int rc = check_state_call(c, &shape);
  if (rc) return rc;
  // instr: the two instrument rows are the last two parameter rows of every ray, here and in the kernel; the sum kernel
  // and the field of view (linear in the rays' band values) take them as they are
  const int n_rays = los->n_rays, n_state = c.col.n_col + c.lev.n_lev + c.row.n_row;
  const int n_hid = c.path ? los->n_gas : 0, n_instr = B.instr ? 2 : 0;
  if (n_state > INT_MAX - 2 - n_hid) return SR_ERR_LIMIT;
  const int n_par = n_state + n_hid + n_instr;
  if (B.fov && n_rays % 3 != 0) return SR_ERR_ARG;
  if ((int64_t)n_rays * (1 + (int64_t)n_par) > INT_MAX) return SR_ERR_LIMIT;
  const int n_spec = n_rays * (1 + n_par);
  // the grid is the descriptor's (a descriptor without one, step <= 0, is refused here)
  rc = lowres_check(n_spec, n_pts, los->g_lo, los->w0, los->step, B.centers_nm, B.widths_nm, B.n_bands, B.n_sigma, B.out_units);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  bool fresh = false;
  rc = lowres_prepare(n_spec, n_pts, los->g_lo, los->w0, los->step, B.centers_nm, B.widths_nm, B.n_bands, B.n_sigma, B.out_units,
                      /*fused=*/true, st, &fresh, B.instr);
  if (rc) return rc;
  rc = limb_jac_state(c, shape, t_lowres.d_weights.p, st);
  if (rc) return rc;
  const size_t low_bytes = sizeof(double) * (size_t)n_spec * B.n_bands;
  rc = t_lowres.s_land.prepare(low_bytes);
  if (rc) return rc;
  LAUNCHCHK(launch_lowres_sum_blocks((int)n_pts, n_spec, B.n_bands, B.out_units, static_cast<double *>(t_lowres.s_land.h),
                                     t_lowres.d_weights.p, st, B.instr));
  HIPCHK(hipStreamSynchronize(st));
  const double *low = static_cast<const double *>(t_lowres.s_land.h);
  if (!n_hid) {
    fov_rows(low, n_rays, n_par, B.n_bands, B.fov, B.out);
    return SR_OK;
  }
  // the pointing row: the hidden per-gas rows added up, in gas order, on the band values that reached the host; the
  // state rows and the instrument rows move as they are
  const int n_out = n_state + 1 + n_instr, nb = B.n_bands;
  std::vector<double> packed((size_t)n_rays * (1 + n_out) * nb);
  std::memcpy(packed.data(), low, sizeof(double) * (size_t)n_rays * nb);
  for (int r = 0; r < n_rays; ++r) {
    const double *src = low + ((size_t)n_rays + (size_t)r * n_par) * nb;
    double *dst = packed.data() + ((size_t)n_rays + (size_t)r * n_out) * nb;
    std::memcpy(dst, src, sizeof(double) * (size_t)n_state * nb);
    double *pt = dst + (size_t)n_state * nb;
    std::memcpy(pt, src + (size_t)n_state * nb, sizeof(double) * nb);
    for (int g = 1; g < n_hid; ++g)
      for (int k = 0; k < nb; ++k) pt[k] = pt[k] + src[(size_t)(n_state + g) * nb + k];
    if (n_instr) std::memcpy(pt + nb, src + (size_t)(n_state + n_hid) * nb, sizeof(double) * (size_t)n_instr * nb);
  }
  fov_rows(packed.data(), n_rays, n_out, nb, B.fov, B.out);
  return SR_OK;
}

// Several level-factored gases.  One level gas is the one-gas entry `twin`, checks and all: the record becomes the one
// that entry fills (a par_lgas that names another gas is refused first: the one-gas entries have no such argument).
static bool one_level_gas_call(StateCall &c, const char *twin, int *rc) {
  *rc = SR_OK;
  if (c.lev.n_lgas != 1 || !c.lev.lgas) return false;
  for (int p = 0; c.lev.par_lgas && p < c.lev.n_lev; ++p)
    if (c.lev.par_lgas[p] != 0) *rc = SR_ERR_ARG;
  c.lev.par_lgas = nullptr;
  c.entry = twin;
  return true;
}

int sr_limb_rays_jac_level_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                               const sr_los_desc *los, int gas, const double *tab, int n_levels, int n_tab_rows,
                               const int32_t *coef_row, int n_par, const int32_t *par_level, const double *par_c,
                               double *rad, double *jac, void *stream) {
  // the state call without column parameters, its checks included: the instances without column code
  const sr_level_gas one = one_level_gas(gas, tab, n_levels, n_tab_rows, coef_row);
  StateCall c{"sr_limb_rays_jac_level_dev", {abs_c, emi_c, n_layers, n_pts, los}, {0, nullptr, nullptr},
              {1, &one, n_par, nullptr, par_level, par_c}, {}, stream};
  c.rad = rad, c.jac = jac;
  return limb_state_spectra(c);
}

int sr_limb_rays_jac_state_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                               const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                               const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                               const int32_t *par_level, const double *par_c, double *rad, double *jac, void *stream) {
  const sr_level_gas one = one_level_gas(gas, tab, n_levels, n_tab_rows, coef_row);
  StateCall c{"sr_limb_rays_jac_state_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {1, &one, n_lev, nullptr, par_level, par_c}, {}, stream};
  c.cols = true, c.rad = rad, c.jac = jac;
  return limb_state_spectra(c);
}

int sr_limb_rays_jac_state_rows_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                    const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                                    const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                                    const int32_t *par_level, const double *par_c, const double *dabs_c, const double *demi_c,
                                    int n_row, const double *par_t, double *rad, double *jac, void *stream) {
  const sr_level_gas one = one_level_gas(gas, tab, n_levels, n_tab_rows, coef_row);
  StateCall c{"sr_limb_rays_jac_state_rows_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {1, &one, n_lev, nullptr, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.rad = rad, c.jac = jac;
  return limb_state_rows(c);
}

int sr_limb_rays_state_bands_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                 const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                                 const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                                 const int32_t *par_level, const double *par_c, const double *dabs_c, const double *demi_c,
                                 int n_row, const double *par_t, const double *centers_nm, const double *widths_nm,
                                 int n_bands, double n_sigma, int out_units, const double *fov, double *out, void *stream) {
  const sr_level_gas one = one_level_gas(gas, tab, n_levels, n_tab_rows, coef_row);
  const StateBands bands{centers_nm, widths_nm, n_bands, n_sigma, out_units, fov, out, /*instr=*/false};
  StateCall c{"sr_limb_rays_state_bands_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {1, &one, n_lev, nullptr, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.bands = &bands;
  return limb_state_bands(c);
}

int sr_limb_rays_jac_state_gases_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                     const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                     const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                     const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                     const double *par_t, double *rad, double *jac, void *stream) {
  StateCall c{"sr_limb_rays_jac_state_gases_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {n_lgas, lgas, n_lev, par_lgas, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.rad = rad, c.jac = jac;
  int rc;
  if (one_level_gas_call(c, "sr_limb_rays_jac_state_rows_dev", &rc)) return rc ? rc : limb_state_rows(c);
  c.cols = n_col > 0;
  return limb_state_spectra(c);
}

int sr_limb_rays_state_bands_gases_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                       const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                       const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                       const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                       const double *par_t, const double *centers_nm, const double *widths_nm, int n_bands,
                                       double n_sigma, int out_units, const double *fov, double *out, void *stream) {
  const StateBands bands{centers_nm, widths_nm, n_bands, n_sigma, out_units, fov, out, /*instr=*/false};
  StateCall c{"sr_limb_rays_state_bands_gases_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {n_lgas, lgas, n_lev, par_lgas, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.bands = &bands;
  int rc;
  one_level_gas_call(c, "sr_limb_rays_state_bands_dev", &rc);
  return rc ? rc : limb_state_bands(c);
}

// ... with the two instrument rows behind the parameters' (d / d band centre, d / d ln ILS width of the radiance's bands):
// the same arguments, the same checks, out [n_rays / 3 or n_rays][1 + n_par + 2][n_bands]; no parameter at all is allowed.
int sr_limb_rays_state_bands_instr_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                       const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                                       const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                                       const int32_t *par_level, const double *par_c, const double *dabs_c, const double *demi_c,
                                       int n_row, const double *par_t, const double *centers_nm, const double *widths_nm,
                                       int n_bands, double n_sigma, int out_units, const double *fov, double *out, void *stream) {
  const sr_level_gas one = one_level_gas(gas, tab, n_levels, n_tab_rows, coef_row);
  const StateBands bands{centers_nm, widths_nm, n_bands, n_sigma, out_units, fov, out, /*instr=*/true};
  StateCall c{"sr_limb_rays_state_bands_instr_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {1, &one, n_lev, nullptr, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.bands = &bands;
  return limb_state_bands(c);
}

int sr_limb_rays_state_bands_instr_gases_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                             const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w,
                                             int n_lgas, const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas,
                                             const int32_t *par_level, const double *par_c, const double *dabs_c,
                                             const double *demi_c, int n_row, const double *par_t, const double *centers_nm,
                                             const double *widths_nm, int n_bands, double n_sigma, int out_units,
                                             const double *fov, double *out, void *stream) {
  const StateBands bands{centers_nm, widths_nm, n_bands, n_sigma, out_units, fov, out, /*instr=*/true};
  StateCall c{"sr_limb_rays_state_bands_instr_gases_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {n_lgas, lgas, n_lev, par_lgas, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.bands = &bands;
  int rc;
  one_level_gas_call(c, "sr_limb_rays_state_bands_instr_dev", &rc);
  return rc ? rc : limb_state_bands(c);
}

// ... with the POINTING derivative, d / d z_t of every ray's own tangent altitude: n_gas hidden column slots whose D rows
// are d col_g / d z_t (stage_los with the path), added up behind the recursion.  The twin entries' records and checks.
static bool path_ok(const sr_los_path *path) { return path && path->alt && path->dx_dz && path->dalt_dz; }

int sr_limb_rays_jac_state_path_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                    const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                    const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                    const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                    const double *par_t, const sr_los_path *path, double *rad, double *jac, void *stream) {
  if (!path_ok(path)) return SR_ERR_ARG;
  StateCall c{"sr_limb_rays_jac_state_path_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {n_lgas, lgas, n_lev, par_lgas, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.rad = rad, c.jac = jac, c.path = path;
  int rc;
  if (one_level_gas_call(c, "sr_limb_rays_jac_state_path_dev", &rc)) {
    if (rc) return rc;
    c.cols = true;
    if (n_row == 0) c.row = StateRows{};
    return limb_state_spectra(c);
  }
  c.cols = true;
  return limb_state_spectra(c);
}

int sr_limb_rays_state_bands_path_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                      const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                      const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                      const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                      const double *par_t, const double *centers_nm, const double *widths_nm, int n_bands,
                                      double n_sigma, int out_units, const double *fov, double *out, void *stream,
                                      int instrument, const sr_los_path *path) {
  if (!path_ok(path)) return SR_ERR_ARG;
  const StateBands bands{centers_nm, widths_nm, n_bands, n_sigma, out_units, fov, out, /*instr=*/instrument != 0};
  StateCall c{"sr_limb_rays_state_bands_path_dev", {abs_c, emi_c, n_layers, n_pts, los}, {n_col, par_gas, par_w},
              {n_lgas, lgas, n_lev, par_lgas, par_level, par_c}, {dabs_c, demi_c, n_row, par_t}, stream};
  c.bands = &bands, c.path = path;
  int rc;
  one_level_gas_call(c, "sr_limb_rays_state_bands_path_dev", &rc);
  return rc ? rc : limb_state_bands(c);
}

int sr_limb_rays_parts_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, const sr_los_desc *los,
                           int gas,const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_part,
                           const int32_t *part_gas, const int32_t *part_level, const double *part_c, double *rad,
                           double *parts, void *stream) {
  // everything is checked here, before the first copy or launch (the LOS too, as sr_limb_rays_jac_level_dev does)
  LosShape shape;
  int rc = check_limb_call(abs_c, emi_c, n_layers, n_pts, part_gas && part_level && parts && n_part >= 1);
  if (rc) return rc;
  if (tab && n_levels > 0 && n_tab_rows > 0 && 2 * (int64_t)n_levels * n_tab_rows > INT_MAX) return SR_ERR_LIMIT; // 32-bit row numbers
  rc = check_los(los, n_layers, &shape);
  if (!rc) rc = refuse_init_mode_1(los, "sr_limb_rays_parts_dev", SR_ERR_ARG);
  if (rc) return rc;
  bool any_level = false;
  for (int k = 0; k < n_part; ++k) {
    if (part_gas[k] < 0 || part_gas[k] >= los->n_gas || part_level[k] < -1) return SR_ERR_ARG;
    if (part_level[k] < 0) continue;
    any_level = true;
    if (part_gas[k] != gas) {
      g_err = "sr_limb_rays_parts_dev: a level part of another gas than the level-factored one";
      return SR_ERR_ARG;
    }
    if (!tab || !coef_row || !part_c || part_level[k] >= n_levels || n_tab_rows <= 0) return SR_ERR_ARG;
  }
  if (any_level && !coef_rows_in_range(coef_row, n_layers, n_tab_rows)) return SR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the parts in level order (stable; gas parts first, the background last), NP slots per block: the slots of one
  // level are neighbours, so a row's table value is loaded once per distinct level
  const int n_slot = n_part + 1, np = limb_parts_np(n_part), n_blocks = (n_slot + np - 1) / np;
  std::vector<int> order = order_by_level(n_part, part_level);
  order.push_back(n_part);
  std::vector<int> slot_level((size_t)n_blocks * np, kPartNoSource), slot_part((size_t)n_blocks * np, -1);
  std::vector<unsigned> words((size_t)n_blocks * n_layers, 0u);
  std::vector<double> cc((size_t)n_blocks * n_layers * np, 0.0);
  for (int i = 0; i < n_slot; ++i) {
    const int k = order[i], b = i / np, q = i % np;
    slot_part[i] = k;
    if (k == n_part) continue; // the background: no source
    slot_level[i] = part_level[k] >= 0 ? (2 * part_level[k] + 1) * n_tab_rows : -1 - part_gas[k];
    for (int r = 0; r < n_layers; ++r) {
      unsigned &w = words[(size_t)b * n_layers + r];
      if (part_level[k] < 0) { // a gas part: active on every row; its coefficient slot carries the gas's index
        w |= 1u << q;
        const int64_t g = part_gas[k];
        std::memcpy(&cc[((size_t)b * n_layers + r) * np + q], &g, sizeof(g));
        continue;
      }
      const double c = part_c[(size_t)k * n_layers + r];
      if (c == 0.0) continue;
      cc[((size_t)b * n_layers + r) * np + q] = c;
      const bool passed_on = q > 0 && slot_level[i - 1] == slot_level[i] && (w >> (q - 1) & 1u);
      w |= 1u << q | (passed_on ? 0u : 1u << (16 + q));
    }
  }
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const auto p_cc = pk.copy(cc.data(), cc.size());
  const auto p_word = pk.copy(words.data(), words.size());
  const auto p_row = any_level ? pk.copy(coef_row, (size_t)n_layers) : pk.zeros<int32_t>((size_t)n_layers);
  const auto p_lev = pk.copy(slot_level.data(), slot_level.size()), p_slot = pk.copy(slot_part.data(), slot_part.size());
  rc = pk.stage(st);
  if (rc) return rc;
  LosDev D;
  rc = stage_los(los, shape, 0, nullptr, nullptr, st, &D);
  if (rc) return rc;
  LAUNCHCHK(launch_limb_parts(abs_c, emi_c, (int)n_pts, n_layers, los->n_rays, D.seg_off, D.seg_layer, D.col,
                              limb_opts(los, D.n_seg), any_level ? gas : 0, tab, pk.dev(p_row), n_blocks, pk.dev(p_word),
                              pk.dev(p_cc), pk.dev(p_lev), pk.dev(p_slot), n_part, rad, parts, st));
  return mark_both(pk.slot(), *D.slot, st);
}

// ------------------------------------------------------------------------
int sr_lut_interp_dev(const double *g_tab, int n_pt, int64_t n_pts, int n_steps, const int32_t *idx4,
                      const double *wgt4, const double *pop, int combine, double *out_a, double *out_e,
                      void *stream) {
  if (!g_tab || !idx4 || !wgt4 || !out_a || n_pt <= 0 || n_pts <= 0 || n_steps <= 0) return SR_ERR_ARG;
  if (combine && (!pop || !out_e)) return SR_ERR_ARG;
  if (n_pts > 2000000) return SR_ERR_LIMIT;
  for (int s = 0; s < n_steps; ++s) {
    const int32_t *q = idx4 + 4 * s;
    const bool bil = q[2] >= 0;
    for (int i = 0; i < 4; ++i) {
      if (!std::isfinite(wgt4[4 * s + i])) return SR_ERR_ARG; // (a planner that divided by T2 - T1 == 0)
      if (!bil && i >= 2) { if (q[i] >= 0) return SR_ERR_ARG; continue; }
      if (q[i] < 0 || q[i] >= n_pt) return SR_ERR_ARG; // would read out of the table
    }
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const auto p_wgt = pk.copy(wgt4, 4 * (size_t)n_steps);
  const auto p_pop = pop ? pk.copy(pop, (size_t)n_steps) : pk.zeros<double>((size_t)n_steps);
  const auto p_idx = pk.copy(idx4, 4 * (size_t)n_steps);
  const int rc = pk.stage(st);
  if (rc) return rc;
  LAUNCHCHK(launch_lut(combine, g_tab, n_pt, (int)n_pts, n_steps, pk.dev(p_idx), pk.dev(p_wgt), pk.dev(p_pop), out_a, out_e, st));
  return pk.slot().mark(st);
}

// ------------------------------------------------------------------------
int sr_hires_to_lowres_dev(const double *rad, int n_rays, int64_t n_pts, double w0, double step,
                           const double *centers_nm, const double *widths_nm, int n_bands, double n_sigma,
                           int out_units, double *out_host, void *stream) {
  return sr_hires_to_lowres_shard_dev(rad, n_rays, n_pts, 0, w0, step, centers_nm, widths_nm, n_bands, n_sigma, out_units,
                                      out_host, stream);
}

int sr_hires_to_lowres_shard_dev(const double *rad, int n_rays, int64_t n_pts, int64_t g_lo, double w0, double step,
                                 const double *centers_nm, const double *widths_nm, int n_bands, double n_sigma,
                                 int out_units, double *out_host, void *stream) {
  if (!rad || !out_host) return SR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool fresh = false;
  int rc = lowres_prepare(n_rays, n_pts, g_lo, w0, step, centers_nm, widths_nm, n_bands, n_sigma, out_units, /*fused=*/false, st, &fresh);
  if (rc) return rc;
  LowresState &L = t_lowres;
  LAUNCHCHK(launch_lowres(rad, (int)n_pts, (int)g_lo, n_rays, w0, step, nullptr, nullptr, n_bands, n_sigma, out_units,
                          L.d_out.as<double>(), L.d_weights.p, st, /*weights=*/false));
  return lowres_land(n_rays, n_bands, out_host, st);
}

// The instrument step with its two instrument derivatives: out_host [n_rays][3][n_bands] = the value (sr_hires_to_lowres_
// shard_dev's, bit for bit), d / d band centre (per nm), d / d ln ILS width; arguments, limits, refusals and status codes
// as sr_hires_to_lowres_shard_dev.
int sr_hires_to_lowres_instr_shard_dev(const double *rad, int n_rays, int64_t n_pts, int64_t g_lo, double w0, double step,
                                       const double *centers_nm, const double *widths_nm, int n_bands, double n_sigma,
                                       int out_units, double *out_host, void *stream) {
  if (!rad || !out_host) return SR_ERR_ARG;
  if (n_rays > INT_MAX / 3) return SR_ERR_LIMIT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool fresh = false;
  int rc = lowres_prepare(n_rays > 0 ? 3 * n_rays : n_rays, n_pts, g_lo, w0, step, centers_nm, widths_nm, n_bands, n_sigma, out_units,
                          /*fused=*/false, st, &fresh, /*instr=*/true);
  if (rc) return rc;
  LowresState &L = t_lowres;
  LAUNCHCHK(launch_lowres_instr(rad, (int)n_pts, n_rays, n_bands, out_units, L.d_out.as<double>(), L.d_weights.p, st));
  return lowres_land(3 * n_rays, n_bands, out_host, st);
}

// The calling thread's instrument line shape: a table of knots (copied here, with its slopes formed once) or, with NULL, the
// Gaussian.  No device call: the next band call's lowres_prepare sends the table up with its bands.  A refused descriptor
// leaves the binding as it was.
int sr_set_ils(const sr_ils_desc *ils) {
  IlsState &I = t_ils;
  if (ils) {
    const int rc = ils_check(ils);
    if (rc) return rc;
    std::vector<double> tab(2 * (size_t)ils->n_shapes * ils->n_tab);
    for (int q = 0; q < ils->n_shapes; ++q) ils_slopes(ils->phi + (size_t)q * ils->n_tab, ils->n_tab, tab.data() + 2 * (size_t)q * ils->n_tab);
    I.tab.swap(tab);
    I.n_shapes = ils->n_shapes; I.n_tab = ils->n_tab; I.t_lo = ils->t_lo; I.t_hi = ils->t_hi;
  } else {
    std::vector<double>().swap(I.tab);
    I.n_shapes = I.n_tab = 0; I.t_lo = I.t_hi = 0.0;
  }
  I.on = ils != nullptr;
  ++I.gen;
  return SR_OK;
}

// The exact integral over t of every table's interpolant: on an interval the cubic Hermite integrates to
// h (phi_k + phi_(k+1)) / 2 + h^2 (m_k - m_(k+1)) / 12; with d = h m the sum is h (trapezoids + (d_0 - d_(n-1)) / 12).
int sr_ils_area(const sr_ils_desc *ils, double *area) {
  if (!ils || !area) return SR_ERR_ARG;
  const int rc = ils_check(ils);
  if (rc) return rc;
  const int n = ils->n_tab;
  const double h = (ils->t_hi - ils->t_lo) / (double)(n - 1);
  for (int q = 0; q < ils->n_shapes; ++q) {
    const double *phi = ils->phi + (size_t)q * n;
    double sum = 0.0;
    for (int k = 0; k + 1 < n; ++k) sum += (phi[k] + phi[k + 1]) / 2.0;
    sum += ((phi[1] - phi[0]) - (phi[n - 1] - phi[n - 2])) / 12.0;
    area[q] = h * sum;
  }
  return SR_OK;
}

} // extern "C"

// A tabulated absorber resident on the device (sr_abs_table_create): the values of all sets in one block, their axes on
// the host (a call stages the descriptors of the sets its rows use with the rows' plan).  Read-only after creation.
struct sr_abs_table {
  static constexpr const char *kName = "sr_abs_table";
  DevBuf d_values;
  std::vector<double> v0, dv;
  std::vector<int64_t> off; // [n_sets + 1]
  int n_sets = 0, dev = -1;
  hipEvent_t ev_last = nullptr; // HandleScope: destroy waits for the last call that reads the values
  bool last_recorded = false;
};

extern "C" {

int sr_abs_table_create(int n_sets, const double *set_temp, const double *set_v0, const double *set_dv, const int64_t *set_off,
                        const double *values, sr_abs_table **out) {
  if (!set_temp || !set_v0 || !set_dv || !set_off || !values || !out || n_sets <= 0) return SR_ERR_ARG;
  if (n_sets > SR_MAX_ABS_SETS) return SR_ERR_LIMIT;
  if (set_off[0] != 0) return SR_ERR_ARG;
  for (int k = 0; k < n_sets; ++k) {
    if (set_off[k + 1] < set_off[k] || set_off[k + 1] - set_off[k] < 2) return SR_ERR_ARG;
    if (set_off[k + 1] > SR_MAX_ABS_VALUES) return SR_ERR_LIMIT;
    if (!(set_dv[k] > 0.0) || !std::isfinite(set_dv[k]) || !std::isfinite(set_v0[k])) return SR_ERR_ARG;
    if (!(set_temp[k] > 0.0) || !std::isfinite(set_temp[k])) return SR_ERR_ARG;
  }
  sr_abs_table *h = new sr_abs_table;
  h->n_sets = n_sets;
  h->v0.assign(set_v0, set_v0 + n_sets);
  h->dv.assign(set_dv, set_dv + n_sets);
  h->off.assign(set_off, set_off + n_sets + 1);
  const size_t bytes = sizeof(double) * (size_t)set_off[n_sets];
  hipError_t e = hipGetDevice(&h->dev);
  int rc = e == hipSuccess ? h->d_values.ensure(bytes) : hip_fail(e, "hipGetDevice");
  if (!rc) {
    e = hipMemcpy(h->d_values.p, values, bytes, hipMemcpyHostToDevice); // (complete on return: every later call may read)
    if (e != hipSuccess) rc = hip_fail(e, "sr_abs_table_create: copy");
  }
  if (rc) {
    h->d_values.release();
    delete h;
    return rc;
  }
  *out = h;
  return SR_OK;
}

int sr_abs_table_destroy(sr_abs_table *h) {
  if (!h) return SR_OK;
  if (h->last_recorded) (void)hipEventSynchronize(h->ev_last);
  h->d_values.release();
  if (h->ev_last) (void)hipEventDestroy(h->ev_last);
  delete h;
  return SR_OK;
}

int sr_abs_table_layers_dev(sr_abs_table *h, int n_rows, const double *temps, const double *scale, const int32_t *set2,
                            const double *w2, const double *dw2, double w0, double step, int64_t g_lo, int64_t n_pts,
                            int source, int accumulate, double *abs_out, double *emi_out, double *dabs_out, double *demi_out,
                            void *stream) {
  if (!h || !temps || !set2 || !w2 || !abs_out || !emi_out || n_rows <= 0 || n_pts <= 0 || g_lo < 0) return SR_ERR_ARG;
  if (dabs_out && !dw2) return SR_ERR_ARG;
  if (source ? (dabs_out != nullptr) != (demi_out != nullptr) : (demi_out && !dabs_out)) return SR_ERR_ARG;
  if (!std::isfinite(w0) || !std::isfinite(step)) return SR_ERR_ARG;
  if (n_pts > 2000000 || g_lo + n_pts > INT32_MAX || n_rows > SR_MAX_ABS_ROWS) return SR_ERR_LIMIT;
  const bool deriv = dabs_out != nullptr;
  for (int r = 0; r < n_rows; ++r) {
    if (!(temps[r] > 0.0) || !std::isfinite(temps[r]) || (scale && !std::isfinite(scale[r]))) return SR_ERR_ARG;
    for (int q = 0; q < 2; ++q) {
      if (set2[2 * r + q] < 0 || set2[2 * r + q] >= h->n_sets) return SR_ERR_ARG; // would read out of the table
      if (!std::isfinite(w2[2 * r + q]) || (deriv && !std::isfinite(dw2[2 * r + q]))) return SR_ERR_ARG;
    }
  }
  // the rows in the caller's order, cut into launches whose rows use at most kAbsTabMaxSets sets between them; slot2:
  // a row's two sets as slots of its launch's list
  struct Group { int row0, row1, n_used; };
  std::vector<Group> groups;
  std::vector<double> g_v0, g_dv;
  std::vector<long long> g_off;
  std::vector<int> g_n, slot2(2 * (size_t)n_rows), used;
  auto close_group = [&](int row0, int row1) {
    groups.push_back(Group{row0, row1, (int)used.size()});
    for (int q = 0; q < kAbsTabMaxSets; ++q) {
      const int k = q < (int)used.size() ? used[(size_t)q] : used[0];
      g_v0.push_back(h->v0[(size_t)k]);
      g_dv.push_back(h->dv[(size_t)k]);
      g_off.push_back((long long)h->off[(size_t)k]);
      g_n.push_back((int)(h->off[(size_t)k + 1] - h->off[(size_t)k]));
    }
    used.clear();
  };
  auto slot_of = [&](int k) { return (int)(std::find(used.begin(), used.end(), k) - used.begin()); };
  int row0 = 0;
  for (int r = 0; r < n_rows; ++r) {
    const int lo = set2[2 * r], hi = set2[2 * r + 1];
    const int fresh = (slot_of(lo) == (int)used.size()) + (hi != lo && slot_of(hi) == (int)used.size());
    if ((int)used.size() + fresh > kAbsTabMaxSets) {
      close_group(row0, r);
      row0 = r;
    }
    for (int q = 0; q < 2; ++q) {
      const int k = set2[2 * r + q];
      if (slot_of(k) == (int)used.size()) used.push_back(k);
      slot2[2 * (size_t)r + q] = slot_of(k);
    }
  }
  close_group(row0, n_rows);
  hipStream_t st = static_cast<hipStream_t>(stream);
  HandleScope<sr_abs_table> scope(h, st);
  int rc = scope.enter();
  if (rc) return rc;
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const size_t n2 = 2 * (size_t)n_rows;
  const auto p_T = pk.copy(temps, (size_t)n_rows), p_c = scale ? pk.copy(scale, (size_t)n_rows) : pk.room<double>((size_t)n_rows);
  const auto p_slot = pk.copy(slot2.data(), n2);
  const auto p_w = pk.copy(w2, n2), p_dw = pk.copy(dw2, deriv ? n2 : 0, 1);
  const auto p_v0 = pk.copy(g_v0.data(), g_v0.size()), p_dv = pk.copy(g_dv.data(), g_dv.size());
  const auto p_off = pk.copy(g_off.data(), g_off.size());
  const auto p_n = pk.copy(g_n.data(), g_n.size());
  rc = pk.prepare();
  if (rc) return rc;
  if (!scale) std::fill(pk.host(p_c), pk.host(p_c) + n_rows, 1.0);
  rc = pk.push_early(st);
  if (rc) return rc;
  for (size_t g = 0; g < groups.size(); ++g) {
    const size_t at = g * kAbsTabMaxSets;
    LAUNCHCHK(launch_absorber_table(groups[g].n_used, pk.dev(p_v0) + at, pk.dev(p_dv) + at, pk.dev(p_off) + at, pk.dev(p_n) + at,
                                    h->d_values.as<double>(), groups[g].row0, groups[g].row1, pk.dev(p_T), pk.dev(p_c), pk.dev(p_slot),
                                    pk.dev(p_w), deriv ? pk.dev(p_dw) : nullptr, w0, step, (int)g_lo, (int)n_pts, source != 0,
                                    accumulate != 0, abs_out, emi_out, dabs_out, demi_out, st));
  }
  rc = pk.slot().mark(st);
  if (rc) return rc;
  return scope.leave();
}

// The single-scattering solar source of coefficient rows (sr_solar_source.hip).  One check of the descriptor for both
// entries: everything the kernel would index with or multiply by is looked at before the first copy or launch.
static thread_local int g_solar_full_lists = 0; // sr_set_solar_full_lists: every chunk listed (a check)
constexpr int64_t kSolarMaxPts = 2000000;         // grid points of a call of the family, solar and diffuse
int sr_set_solar_full_lists(int on) {
  g_solar_full_lists = on != 0;
  return SR_OK;
}

static int check_solar_desc(const sr_solar_desc *d, int n_k, int n_src, std::vector<int> *tile_off, std::vector<int> *chunks) {
  if (!d || !d->u || !d->w || !d->src_row || d->n_rows <= 0 || n_k <= 0) return SR_ERR_ARG;
  if (d->n_rows > SR_MAX_ABS_ROWS || (int64_t)d->n_rows * n_k > SR_MAX_SOLAR_VALUES) return SR_ERR_LIMIT;
  for (int r = 0; r < d->n_rows; ++r) {
    if (!(d->w[r] >= 0.0) || !std::isfinite(d->w[r])) return SR_ERR_ARG;
    if (n_src >= 0 && (d->src_row[r] < 0 || d->src_row[r] >= n_src)) return SR_ERR_ARG; // would read out of sca_abs
  }
  // u is walked once: its check and the chunk lists together (it is the one large array of a call)
  return solar_chunk_lists(d->u, d->w, d->n_rows, n_k, g_solar_full_lists != 0, *tile_off, *chunks) ? SR_OK : SR_ERR_ARG;
}

// The two *_chunk_lists entries: the lists `check` makes of the descriptor, copied out.
static int export_chunk_lists(int32_t *tile_off, int32_t *chunks, int32_t *n_listed,
                              const std::function<int(std::vector<int> *, std::vector<int> *)> &check) {
  if (!tile_off || !chunks || !n_listed) return SR_ERR_ARG;
  std::vector<int> off, ch;
  const int rc = check(&off, &ch);
  if (rc) return rc;
  std::copy(off.begin(), off.end(), tile_off);
  std::copy(ch.begin(), ch.end(), chunks);
  *n_listed = (int32_t)ch.size();
  return SR_OK;
}

// One writer per element: a row of jac belongs to one parameter.
static int check_par_slots(const int32_t *par_slot, int n_par, int n_jac_rows) {
  std::vector<int> slots(par_slot, par_slot + n_par);
  std::sort(slots.begin(), slots.end());
  if (slots.front() < 0 || slots.back() >= n_jac_rows || std::adjacent_find(slots.begin(), slots.end()) != slots.end()) return SR_ERR_ARG;
  return SR_OK;
}

int sr_solar_chunk_lists(const sr_solar_desc *desc, int n_k, int32_t *tile_off, int32_t *chunks, int32_t *n_listed) {
  return export_chunk_lists(tile_off, chunks, n_listed, [&](std::vector<int> *off, std::vector<int> *ch) {
    return check_solar_desc(desc, n_k, -1, off, ch);
  });
}

int sr_solar_source_rows_dev(const sr_solar_desc *desc, const double *tab_abs, int n_k, const double *sca_abs, int n_src,
                             const double *sun, int64_t n_pts, int accumulate, double *emi_out, double *trans_out, void *stream) {
  if (!tab_abs || !sca_abs || !sun || !emi_out || n_src <= 0 || n_pts <= 0) return SR_ERR_ARG;
  if (n_pts > kSolarMaxPts) return SR_ERR_LIMIT;
  std::vector<int> tile_off, chunks;
  int rc = check_solar_desc(desc, n_k, n_src, &tile_off, &chunks);
  if (rc) return rc;
  const int n_rows = desc->n_rows;
  hipStream_t st = static_cast<hipStream_t>(stream);
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const auto p_u = pk.copy(desc->u, (size_t)n_rows * n_k), p_w = pk.copy(desc->w, (size_t)n_rows);
  const auto p_src = pk.copy(desc->src_row, (size_t)n_rows);
  const auto p_off = pk.copy(tile_off.data(), tile_off.size()), p_ch = pk.copy(chunks.data(), chunks.size(), 1);
  rc = pk.stage(st);
  if (rc) return rc;
  LAUNCHCHK(launch_solar_source(tab_abs, n_k, (int)n_pts, pk.dev(p_u), pk.dev(p_w), pk.dev(p_src), n_rows, pk.dev(p_off),
                                pk.dev(p_ch), sca_abs, sun, accumulate != 0, emi_out, trans_out, st));
  return pk.slot().mark(st);
}

// The solar attenuation in the Jacobians (sr_solar_jac.inc).  One check of the descriptor for both entries, as above.
static int check_solar_jac_desc(const sr_solar_jac_desc *d, int n_k, std::vector<int> *tile_off, std::vector<int> *chunks) {
  if (!d || !d->du || d->n_par <= 0 || d->n_rows <= 0 || n_k <= 0) return SR_ERR_ARG;
  if (d->n_rows > SR_MAX_ABS_ROWS || (int64_t)d->n_par * d->n_rows * n_k > SR_MAX_SOLAR_VALUES) return SR_ERR_LIMIT;
  // du is walked once: its check and the chunk lists together
  return solar_jac_chunk_lists(d->du, d->n_par, d->n_rows, n_k, g_solar_full_lists != 0, *tile_off, *chunks) ? SR_OK : SR_ERR_ARG;
}

int sr_solar_jacobian_chunk_lists(const sr_solar_jac_desc *desc, int n_k, int32_t *tile_off, int32_t *chunks, int32_t *n_listed) {
  return export_chunk_lists(tile_off, chunks, n_listed, [&](std::vector<int> *off, std::vector<int> *ch) {
    return check_solar_jac_desc(desc, n_k, off, ch);
  });
}

int sr_solar_jacobian_rows_dev(const sr_solar_jac_desc *desc, const double *tab_abs, int n_k, const double *q, int n_rays,
                               int64_t n_pts, const int32_t *par_slot, double *jac, int n_jac_rows, int accumulate, void *stream) {
  if (!tab_abs || !q || !par_slot || !jac || n_rays <= 0 || n_pts <= 0 || n_jac_rows <= 0) return SR_ERR_ARG;
  if (n_pts > kSolarMaxPts) return SR_ERR_LIMIT;
  std::vector<int> tile_off, chunks;
  int rc = check_solar_jac_desc(desc, n_k, &tile_off, &chunks);
  if (rc) return rc;
  const int n_par = desc->n_par, n_rows = desc->n_rows;
  rc = check_par_slots(par_slot, n_par, n_jac_rows);
  if (rc) return rc;
  // the grid: point blocks (rounded up to eight) x parameters x ray groups
  const int64_t n_blocks = (((n_pts + 255) / 256 + 7) / 8 * 8) * (int64_t)n_par * ((n_rays + kSolarJacRays - 1) / kSolarJacRays);
  if (n_blocks > 2147483647) return SR_ERR_LIMIT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const auto p_du = pk.copy(desc->du, (size_t)n_par * n_rows * n_k);
  const auto p_slot = pk.copy(par_slot, (size_t)n_par);
  const auto p_off = pk.copy(tile_off.data(), tile_off.size()), p_ch = pk.copy(chunks.data(), chunks.size(), 1);
  rc = pk.stage(st);
  if (rc) return rc;
  LAUNCHCHK(launch_solar_jac(tab_abs, n_k, (int)n_pts, pk.dev(p_du), n_par, n_rows, pk.dev(p_off), pk.dev(p_ch), q, n_rays,
                             pk.dev(p_slot), accumulate != 0, jac, n_jac_rows, st));
  return pk.slot().mark(st);
}

// The two-stream diffuse field of coefficient rows (sr_diffuse_source.inc).  The upward sweep's workspace, four doubles
// per (layer, point), comes from a grow-only buffer per (thread, device); a call whose workspace would pass
// kDiffuseWsBytes is made in point chunks, one launch after the other on `stream`.
constexpr size_t kDiffuseWsBytes = (size_t)256 << 20;
static DevBuf &diffuse_workspace(int dev) { // shared by the source and its Jacobian: one per device this thread has used
  static thread_local std::map<int, DevBuf> ws_pool;
  return ws_pool[dev];
}

// The state of a two-stream call, for the source and its Jacobian: mu0 and the albedo, then -- `sized`: n_gas and
// n_layers are inside the limits, so that the arrays may be walked and coef has room -- ssa and asym gas by gas and the
// columns v >= 0.  coef [3][kDiffuseGases]: ssa (1 - f), 1 - ssa, ssa (asym - f), zeros beyond n_gas; w_out: out_gas's
// ssa (1 - f) (0 without one).
static int check_diffuse_desc(const sr_diffuse_desc *d, bool sized, int out_gas, double (&coef)[3 * kDiffuseGases], double *w_out) {
  if (!(d->mu0 >= -1.0 && d->mu0 <= 1.0) || !(d->surface_albedo >= 0.0 && d->surface_albedo <= 1.0)) return SR_ERR_ARG;
  std::fill(coef, coef + 3 * kDiffuseGases, 0.0);
  *w_out = 0.0;
  if (!sized) return SR_OK;
  for (int g = 0; g < d->n_gas; ++g) {
    const double ssa = d->ssa[g], as = d->asym[g];
    if (!(ssa >= 0.0 && ssa <= 1.0) || !(as >= -0.5 && as < 1.0)) return SR_ERR_ARG; // (a NaN fails both)
    const double f = as > 0.0 ? as * as : 0.0;
    coef[g] = ssa * (1.0 - f);
    coef[kDiffuseGases + g] = 1.0 - ssa;
    coef[2 * kDiffuseGases + g] = ssa * (as - f);
    if (g == out_gas) *w_out = coef[g];
  }
  for (size_t i = 0; i < (size_t)d->n_gas * d->n_layers; ++i)
    if (!(d->v[i] >= 0.0) || !std::isfinite(d->v[i])) return SR_ERR_ARG;
  return SR_OK;
}

// Points per launch and, for the Jacobian, parameter tiles per launch of a call whose workspace takes `per` bytes per
// (tile, point): whole blocks of 256 points inside kDiffuseWsBytes (one block at the least), then as many tiles as fit.
struct DiffuseChunks { int chunk, tiles; };
static DiffuseChunks diffuse_chunks(size_t per, int64_t n_pts, int n_tiles) {
  const int pts_max = (int)std::max<size_t>(256, kDiffuseWsBytes / per / 256 * 256);
  const int chunk = (int)std::min<int64_t>(pts_max, (n_pts + 255) / 256 * 256);
  const int tiles = (int)std::min<size_t>((size_t)n_tiles, std::max<size_t>(1, kDiffuseWsBytes / (per * (size_t)chunk)));
  return DiffuseChunks{chunk, tiles};
}

// What the three forward entries ask of their arguments alike, in the order of their refusals: the pointers and sizes
// (with `bad`, the entry's own argument rules), the limits (with `over`, the entry's own), out_gas against emi_out, and
// that something is asked for.
static int check_diffuse_field_args(const sr_diffuse_desc *desc, const double *tab_abs, int64_t n_pts, bool bad, bool over,
                                    int out_gas, const double *emi_out, const double *j_out, const double *flux_out) {
  if (!desc || !desc->v || !desc->ssa || !desc->asym || !tab_abs || bad) return SR_ERR_ARG;
  if (desc->n_gas <= 0 || desc->n_layers <= 0 || n_pts <= 0) return SR_ERR_ARG;
  if (desc->n_gas > kDiffuseGases || desc->n_layers > SR_MAX_ABS_ROWS || n_pts > kSolarMaxPts || over) return SR_ERR_LIMIT;
  if (out_gas < -1 || out_gas >= desc->n_gas || (out_gas < 0) != (emi_out == nullptr)) return SR_ERR_ARG;
  if (!emi_out && !j_out && !flux_out) return SR_ERR_ARG;
  return SR_OK;
}

// What the three forward entries share once their arguments are checked: the workspace of `per` bytes per point, the
// staging of v and coef with the parts the entry adds (parts(pk)), and the point chunks, one launch after the other on
// `stream`: launch(pk, p_lo, p_hi, ws, chunk, v, coef, st).  ring is the entry's own, so that no entry waits for
// another's slots.
using DiffuseLaunch = std::function<int(StagePack &, int, int, double *, int, const double *, const double *, hipStream_t)>;
static int diffuse_field_run(const sr_diffuse_desc *desc, const double (&coef)[3 * kDiffuseGases], size_t per, int64_t n_pts,
                             StagerRing &ring, void *stream, const std::function<void(StagePack &)> &parts,
                             const DiffuseLaunch &launch) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int chunk = diffuse_chunks(per, n_pts, 1).chunk;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  DevBuf &ws = diffuse_workspace(dev);
  int rc = ws.ensure(per * (size_t)chunk);
  if (rc) return rc;
  StagePack pk(ring.take());
  const auto p_v = pk.copy(desc->v, (size_t)desc->n_gas * desc->n_layers), p_c = pk.copy(coef, (size_t)3 * kDiffuseGases);
  parts(pk);
  rc = pk.stage(st);
  if (rc) return rc;
  for (int64_t p_lo = 0; p_lo < n_pts; p_lo += chunk) {
    const int p_hi = (int)std::min<int64_t>(n_pts, p_lo + chunk);
    LAUNCHCHK(launch(pk, (int)p_lo, p_hi, ws.as<double>(), chunk, pk.dev(p_v), pk.dev(p_c), st));
  }
  return pk.slot().mark(st);
}

int sr_diffuse_source_rows_dev(const sr_diffuse_desc *desc, const double *tab_abs, const double *beam, const double *sun,
                               int64_t n_pts, int out_gas, int accumulate, double *emi_out, double *j_out, double *flux_out,
                               void *stream) {
  int rc = check_diffuse_field_args(desc, tab_abs, n_pts, !beam || !sun, false, out_gas, emi_out, j_out, flux_out);
  if (rc) return rc;
  const int n_gas = desc->n_gas, n_layers = desc->n_layers;
  double coef[3 * kDiffuseGases], w_out;
  rc = check_diffuse_desc(desc, true, out_gas, coef, &w_out);
  if (rc) return rc;
  static thread_local StagerRing ring;
  return diffuse_field_run(
      desc, coef, (size_t)32 * n_layers, n_pts, ring, stream, [](StagePack &) {},
      [&](StagePack &, int p_lo, int p_hi, double *ws, int chunk, const double *v, const double *c, hipStream_t st) {
        return launch_diffuse_field(tab_abs, n_gas, n_layers, (int)n_pts, p_lo, p_hi, v, c, nullptr, beam, sun, desc->mu0,
                                    desc->surface_albedo, 0.0, 0.0, 0.0, 0, false, out_gas, ws, chunk, accumulate != 0, emi_out,
                                    j_out, flux_out, st);
      });
}

// Thermal emission as a source of the same field, alone (beam and sun NULL: desc's mu0 is not read) or with the sun's.
// The layers' temperatures are staged with v.
int sr_diffuse_thermal_rows_dev(const sr_diffuse_desc *desc, const sr_diffuse_thermal_desc *th, const double *tab_abs,
                                const double *beam, const double *sun, int64_t n_pts, int out_gas, int accumulate,
                                double *emi_out, double *j_out, double *flux_out, void *stream) {
  const bool bad = !th || !th->temps || (beam == nullptr) != (sun == nullptr) || th->g_lo < 0;
  int rc = check_diffuse_field_args(desc, tab_abs, n_pts, bad, !bad && th->g_lo > INT32_MAX - n_pts, out_gas, emi_out, j_out,
                                    flux_out);
  if (rc) return rc;
  const int n_gas = desc->n_gas, n_layers = desc->n_layers;
  if (th->own_emission && !emi_out) return SR_ERR_ARG;
  if (!(th->t_surface >= 0.0) || !std::isfinite(th->t_surface) || !std::isfinite(th->w0) || !std::isfinite(th->step)) return SR_ERR_ARG;
  for (int l = 0; l < n_layers; ++l)
    if (!(th->temps[l] > 0.0) || !std::isfinite(th->temps[l])) return SR_ERR_ARG;
  sr_diffuse_desc state = *desc;
  if (!beam) state.mu0 = 0.0;
  double coef[3 * kDiffuseGases], w_out;
  rc = check_diffuse_desc(&state, true, out_gas, coef, &w_out);
  if (rc) return rc;
  static thread_local StagerRing ring;
  StagePack::Part<double> p_t{};
  return diffuse_field_run(
      desc, coef, (size_t)32 * n_layers, n_pts, ring, stream, [&](StagePack &pk) { p_t = pk.copy(th->temps, (size_t)n_layers); },
      [&](StagePack &pk, int p_lo, int p_hi, double *ws, int chunk, const double *v, const double *c, hipStream_t st) {
        return launch_diffuse_field(tab_abs, n_gas, n_layers, (int)n_pts, p_lo, p_hi, v, c, pk.dev(p_t), beam, sun, state.mu0,
                                    state.surface_albedo, th->t_surface, th->w0, th->step, (int)th->g_lo, th->own_emission != 0,
                                    out_gas, ws, chunk, accumulate != 0, emi_out, j_out, flux_out, st);
      });
}

// The solar field for several columns of illumination, and the rows of LOS steps (sr_diffuse_columns.inc).  The workspace
// takes 2 + 2 NC doubles per (layer, point) for the instance NC the call runs; the plan -- mu0 and col_w padded to NC, the
// rows sorted by layer -- is diffuse_columns_plan's (sr_solar_plan.hpp), staged with v and the coefficients.
int sr_diffuse_source_columns_dev(const sr_diffuse_desc *desc, const sr_diffuse_columns_desc *cols, const double *tab_abs,
                                  const double *beam, const double *sun, int64_t n_pts, const double *sca_abs, int n_src,
                                  int out_gas, int accumulate, double *emi_out, double *j_out, double *flux_out, void *stream) {
  const bool bad = !cols || !cols->mu0 || !beam || !sun || cols->n_col <= 0 || cols->n_rows < 0 ||
                   (cols->n_rows > 0 && (!cols->col_w || !cols->row_layer || !cols->src_row || !sca_abs || n_src <= 0));
  const bool over = !bad && (cols->n_col > SR_MAX_DIFFUSE_COLUMNS || cols->n_rows > SR_MAX_ABS_ROWS);
  int rc = check_diffuse_field_args(desc, tab_abs, n_pts, bad, over, out_gas, emi_out, j_out, flux_out);
  if (rc) return rc;
  const int n_gas = desc->n_gas, n_layers = desc->n_layers, n_col = cols->n_col, n_rows = cols->n_rows;
  if ((n_rows == 0) != (emi_out == nullptr)) return SR_ERR_ARG;
  sr_diffuse_desc state = *desc;
  state.mu0 = 0.0; // (desc->mu0 is not read: the columns bring their own)
  double coef[3 * kDiffuseGases], w_out;
  rc = check_diffuse_desc(&state, true, out_gas, coef, &w_out);
  if (rc) return rc;
  std::vector<double> mu0p, wp;
  std::vector<int> row_off, row_ix;
  if (!diffuse_columns_plan(cols->mu0, cols->col_w, cols->row_layer, cols->src_row, n_col, n_rows, n_layers, n_src, w_out == 0.0,
                            accumulate != 0, mu0p, wp, row_off, row_ix))
    return SR_ERR_ARG;
  static thread_local StagerRing ring;
  StagePack::Part<double> p_mu{}, p_w{};
  StagePack::Part<int> p_off{}, p_ix{}, p_src{};
  return diffuse_field_run(
      desc, coef, (size_t)8 * (2 + 2 * diffuse_columns_instance(n_col)) * n_layers, n_pts, ring, stream,
      [&](StagePack &pk) {
        p_mu = pk.copy(mu0p.data(), mu0p.size()), p_w = pk.copy(wp.data(), wp.size(), 1);
        p_off = pk.copy(row_off.data(), row_off.size()), p_ix = pk.copy(row_ix.data(), row_ix.size(), 1);
        p_src = pk.copy(cols->src_row, (size_t)n_rows, 1);
      },
      [&](StagePack &pk, int p_lo, int p_hi, double *ws, int chunk, const double *v, const double *c, hipStream_t st) {
        return launch_diffuse_columns(tab_abs, n_gas, n_layers, (int)n_pts, p_lo, p_hi, v, c, beam, n_col, sun, pk.dev(p_mu),
                                      desc->surface_albedo, w_out, pk.dev(p_off), pk.dev(p_ix), pk.dev(p_src), pk.dev(p_w), sca_abs,
                                      ws, chunk, accumulate != 0, emi_out, j_out, flux_out, st);
      });
}

// What the two Jacobian entries share once their arguments are checked: par_slot's check, the workspace, the staging and
// the launches (the entry's comment below).  dir is the direction as its kernel instance reads it: dv
// [n_par][n_gas][n_layers], or -- optics -- dopt [n_par][kDiffuseOpt] (sr_diffuse_optics_jacobian_rows_dev); mask is that
// direction's plan.
static int diffuse_jacobian_run(const sr_diffuse_desc *desc, const double (&coef)[3 * kDiffuseGases], int n_par,
                                const std::vector<int> &mask, const double *dir, bool optics, const double *tab_abs,
                                const double *beam, const double *sun, const double *dlnbeam, const double *q, int n_rays,
                                int64_t n_pts, const int32_t *par_slot, double *jac, int n_jac_rows, int accumulate,
                                double *dj_out, void *stream) {
  const int n_gas = desc->n_gas, n_layers = desc->n_layers;
  int rc = jac ? check_par_slots(par_slot, n_par, n_jac_rows) : SR_OK;
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the workspace: doubles per (tile, layer, point), then points per launch, then tiles per launch
  const bool dj_ws = jac && !dj_out;
  const size_t per = (size_t)8 * n_layers * (3 + 4 * kDiffuseJacPars + (dj_ws ? kDiffuseJacPars : 0));
  const int n_tiles = (n_par + kDiffuseJacPars - 1) / kDiffuseJacPars;
  const DiffuseChunks dc = diffuse_chunks(per, n_pts, n_tiles);
  const int chunk = dc.chunk, tiles = dc.tiles;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  DevBuf &ws = diffuse_workspace(dev);
  rc = ws.ensure(per * (size_t)chunk * tiles);
  if (rc) return rc;
  static thread_local StagerRing ring;
  StagePack pk(ring.take());
  const auto p_v = pk.copy(desc->v, (size_t)n_gas * n_layers), p_c = pk.copy(coef, (size_t)3 * kDiffuseGases);
  const auto p_dir = pk.copy(dir, (size_t)n_par * (optics ? (size_t)kDiffuseOpt : (size_t)n_gas * n_layers));
  const auto p_m = pk.copy(mask.data(), mask.size());
  const auto p_slot = pk.copy(par_slot, jac ? (size_t)n_par : 0, 1);
  rc = pk.stage(st);
  if (rc) return rc;
  double *sweep = ws.as<double>();
  double *dj_room = sweep + (size_t)tiles * (3 + 4 * kDiffuseJacPars) * n_layers * chunk; // (used with dj_ws only)
  for (int64_t p_lo = 0; p_lo < n_pts; p_lo += chunk) {
    const int p_hi = (int)std::min<int64_t>(n_pts, p_lo + chunk);
    for (int t0 = 0; t0 < n_tiles; t0 += tiles) {
      const int par_lo = t0 * kDiffuseJacPars, par_hi = std::min(n_par, (t0 + tiles) * kDiffuseJacPars);
      double *dj = dj_ws ? dj_room : dj_out;
      const int dj_stride = dj_ws ? chunk : (int)n_pts, dj_joff = dj_ws ? (int)p_lo : 0, dj_par0 = dj_ws ? par_lo : 0;
      if (!optics)
        LAUNCHCHK(launch_diffuse_tangent(tab_abs, n_gas, n_layers, (int)n_pts, (int)p_lo, p_hi, par_lo, par_hi, pk.dev(p_v),
                                         pk.dev(p_dir), pk.dev(p_c), pk.dev(p_m), beam, sun, dlnbeam, desc->mu0, desc->surface_albedo,
                                         sweep, chunk, dj, dj_stride, dj_joff, dj_par0, st));
      else
        LAUNCHCHK(launch_diffuse_optics_tangent(tab_abs, n_gas, n_layers, (int)n_pts, (int)p_lo, p_hi, par_lo, par_hi, pk.dev(p_v),
                                                pk.dev(p_dir), pk.dev(p_c), pk.dev(p_m), beam, sun, dlnbeam, desc->mu0,
                                                desc->surface_albedo, sweep, chunk, dj, dj_stride, dj_joff, dj_par0, st));
      if (jac)
        LAUNCHCHK(launch_diffuse_contract(q, n_rays, n_layers, (int)n_pts, (int)p_lo, p_hi, par_lo, par_hi, dj, dj_stride, dj_joff,
                                          dj_par0, pk.dev(p_slot), accumulate != 0, jac, n_jac_rows, st));
    }
  }
  return pk.slot().mark(st);
}

// The diffuse rows in the Jacobians (sr_diffuse_jac.inc).  The workspace is the source's: per (parameter tile, point)
// 3 + 4 kDiffuseJacPars doubles per layer for the two sweeps and, where the caller takes no dj_out, kDiffuseJacPars more
// for the dJ rows the contraction reads; a call whose workspace would pass kDiffuseWsBytes is made in point chunks and
// groups of parameter tiles, a tangent launch and a contraction launch each, one after the other on `stream`.
int sr_diffuse_jacobian_rows_dev(const sr_diffuse_desc *desc, const sr_diffuse_jac_desc *jdesc, const double *tab_abs,
                                 const double *beam, const double *sun, const double *dlnbeam, const double *q, int n_rays,
                                 int64_t n_pts, const int32_t *par_slot, double *jac, int n_jac_rows, int accumulate,
                                 double *dj_out, void *stream) {
  if (!desc || !desc->v || !desc->ssa || !desc->asym || !jdesc || !jdesc->dv || !tab_abs || !beam || !sun) return SR_ERR_ARG;
  if (desc->n_gas <= 0 || desc->n_layers <= 0 || n_pts <= 0 || jdesc->n_par <= 0) return SR_ERR_ARG;
  if ((q == nullptr) != (jac == nullptr) || (!jac && !dj_out)) return SR_ERR_ARG; // q and jac come together; something is asked for
  if (jac && (!par_slot || n_rays <= 0 || n_jac_rows <= 0)) return SR_ERR_ARG;
  const int64_t n_gas64 = desc->n_gas, n_layers64 = desc->n_layers, n_par64 = jdesc->n_par;
  // (the sizes are bounded before the arrays they describe are walked; the limits are reported after dv's check)
  const bool too_large = n_gas64 > kDiffuseGases || n_layers64 > SR_MAX_ABS_ROWS || n_pts > kSolarMaxPts ||
                         n_par64 * n_gas64 * n_layers64 > SR_MAX_SOLAR_VALUES;
  double coef[3 * kDiffuseGases], w_out;
  int rc = check_diffuse_desc(desc, !too_large, -1, coef, &w_out);
  if (rc) return rc;
  std::vector<int> mask;
  if (!too_large && !diffuse_jac_masks(desc->v, jdesc->dv, jdesc->n_par, desc->n_gas, desc->n_layers, mask)) return SR_ERR_ARG;
  if (too_large) return SR_ERR_LIMIT;
  return diffuse_jacobian_run(desc, coef, jdesc->n_par, mask, jdesc->dv, false, tab_abs, beam, sun, dlnbeam, q, n_rays, n_pts,
                              par_slot, jac, n_jac_rows, accumulate, dj_out, stream);
}

// The diffuse rows along a direction in the optics (sr_diffuse_tangent_kernel<NP, true>, sr_diffuse_jac.inc): the argument
// rules, the order of the checks and the limits of sr_diffuse_jacobian_rows_dev, with (dssa, dasym, dalb) in dv's place.
int sr_diffuse_optics_jacobian_rows_dev(const sr_diffuse_desc *desc, const sr_diffuse_optics_desc *odesc, const double *tab_abs,
                                        const double *beam, const double *sun, const double *dlnbeam, const double *q, int n_rays,
                                        int64_t n_pts, const int32_t *par_slot, double *jac, int n_jac_rows, int accumulate,
                                        double *dj_out, void *stream) {
  if (!desc || !desc->v || !desc->ssa || !desc->asym || !odesc || (!odesc->dssa && !odesc->dasym && !odesc->dalb) || !tab_abs ||
      !beam || !sun)
    return SR_ERR_ARG;
  if (desc->n_gas <= 0 || desc->n_layers <= 0 || n_pts <= 0 || odesc->n_par <= 0) return SR_ERR_ARG;
  if ((q == nullptr) != (jac == nullptr) || (!jac && !dj_out)) return SR_ERR_ARG;
  if (jac && (!par_slot || n_rays <= 0 || n_jac_rows <= 0)) return SR_ERR_ARG;
  const int64_t n_gas64 = desc->n_gas, n_layers64 = desc->n_layers, n_par64 = odesc->n_par;
  const bool too_large = n_gas64 > kDiffuseGases || n_layers64 > SR_MAX_ABS_ROWS || n_pts > kSolarMaxPts ||
                         n_par64 * n_gas64 * n_layers64 > SR_MAX_SOLAR_VALUES;
  double coef[3 * kDiffuseGases], w_out;
  int rc = check_diffuse_desc(desc, !too_large, -1, coef, &w_out);
  if (rc) return rc;
  std::vector<double> dopt;
  std::vector<int> mask;
  if (!too_large && !diffuse_optics_plan(desc->v, desc->ssa, desc->asym, odesc->dssa, odesc->dasym, odesc->dalb, odesc->n_par,
                                         desc->n_gas, desc->n_layers, dopt, mask))
    return SR_ERR_ARG;
  if (too_large) return SR_ERR_LIMIT;
  return diffuse_jacobian_run(desc, coef, odesc->n_par, mask, dopt.data(), true, tab_abs, beam, sun, dlnbeam, q, n_rays, n_pts,
                              par_slot, jac, n_jac_rows, accumulate, dj_out, stream);
}

// ------------------------------------------------------------------------
// f2py-shaped shims (host pointers)
// ------------------------------------------------------------------------
int sr_humliv_bb(const double *x, int n, int i1, int i2, double x0, double lw, double dw, double *y) {
  if (!x || !y || n < 2) return SR_ERR_ARG;
  if (i1 > i2 || i1 < 1 || i2 > n) return SR_ERR_ARG; // lineshape.f:253-256
  if (!(dw > 0.0)) return SR_ERR_ARG;                  // lineshape.f:260-264
  if (i2 - i1 + 1 > 32767) return SR_ERR_LIMIT;        // window indices are 16-bit (imxsig = 13010)
  if (i2 - i1 < 1) return SR_ERR_ARG;
  const int outer = !(x[i1 - 1] < x0 && x0 < x[i2 - 1]); // lineshape.f:272, 358
  DevBuf dx, dy;
  int rc = dx.ensure(sizeof(double) * n);
  if (!rc) rc = dy.ensure(sizeof(double) * n);
  if (rc) { dx.release(); dy.release(); return rc; }
  hipError_t e = hipMemcpy(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dy.p, 0, sizeof(double) * n);
  if (e == hipSuccess)
    e = (hipError_t)launch_humliv(dx.as<double>(), i1, i2, x0, lw, dw, dy.as<double>(), outer, nullptr);
  if (e == hipSuccess) e = hipMemcpy(y, dy.p, sizeof(double) * n, hipMemcpyDeviceToHost);
  dx.release();
  dy.release();
  return e == hipSuccess ? SR_OK : hip_fail(e, "sr_humliv_bb");
}

int sr_sum_all_lines(double *spe, int64_t n_spe, const double *rows, const int32_t *init, const int32_t *fin,
                     int n_lines, int row_len) {
  if (!spe || n_spe <= 0 || n_lines < 0 || row_len <= 0) return SR_ERR_ARG;
  if (n_lines > 0 && (!rows || !init || !fin)) return SR_ERR_ARG;
  if (n_spe > 2000000) return SR_ERR_LIMIT; // imxsig_long
  for (int l = 0; l < n_lines; ++l)           // the Fortran would write out of bounds
    if (init[l] < 1 || fin[l] > n_spe || fin[l] - init[l] + 1 > row_len) return SR_ERR_ARG;
  if (n_lines == 0) return SR_OK;
  DevBuf ds, dr, di;
  const size_t b_rows = sizeof(double) * (size_t)n_lines * row_len;
  int rc = ds.ensure(sizeof(double) * n_spe);
  if (!rc) rc = dr.ensure(b_rows);
  if (!rc) rc = di.ensure(sizeof(int) * 2 * (size_t)n_lines);
  hipError_t e = hipSuccess;
  if (!rc) {
    e = hipMemcpy(ds.p, spe, sizeof(double) * n_spe, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dr.p, rows, b_rows, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(di.p, init, sizeof(int) * n_lines, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(di.as<int>() + n_lines, fin, sizeof(int) * n_lines, hipMemcpyHostToDevice);
    if (e == hipSuccess)
      e = (hipError_t)launch_sum_lines(ds.as<double>(), (long)n_spe, dr.as<double>(), di.as<int>(),
                                       di.as<int>() + n_lines, n_lines, row_len, nullptr);
    if (e == hipSuccess) e = hipMemcpy(spe, ds.p, sizeof(double) * n_spe, hipMemcpyDeviceToHost);
  }
  ds.release(); dr.release(); di.release();
  if (rc) return rc;
  return e == hipSuccess ? SR_OK : hip_fail(e, "sr_sum_all_lines");
}

int sr_curgod(int which, const double *nd, const double *vmr, const double *f, const double *x,
              const int32_t *off, int n_seg, double *res) {
  if (which < 1 || which > 4 || !nd || !x || !off || !res || n_seg < 0) return SR_ERR_ARG;
  if (which >= 2 && !vmr) return SR_ERR_ARG;
  if (which >= 3 && !f) return SR_ERR_ARG;
  if (n_seg == 0) return SR_OK;
  if (off[0] != 0) return SR_ERR_ARG;
  for (int s = 0; s < n_seg; ++s) {
    if (off[s + 1] < off[s]) return SR_ERR_ARG;
    if (off[s + 1] - off[s] > 8000) return SR_ERR_LIMIT; // imxstp, parameters.inc:64
  }
  const size_t n = (size_t)off[n_seg];
  const int narr = which == 1 ? 2 : (which == 2 ? 3 : 4);
  DevBuf d, dofs, dres;
  int rc = d.ensure(sizeof(double) * std::max<size_t>(n, 1) * narr);
  if (!rc) rc = dofs.ensure(sizeof(int) * (size_t)(n_seg + 1));
  if (!rc) rc = dres.ensure(sizeof(double) * (size_t)n_seg);
  hipError_t e = hipSuccess;
  if (!rc) {
    double *b = d.as<double>();
    const double *srcs[4] = {nd, x, vmr, f};
    for (int a = 0; a < narr && e == hipSuccess; ++a)
      if (n) e = hipMemcpy(b + a * n, srcs[a], sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dofs.p, off, sizeof(int) * (size_t)(n_seg + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess)
      e = (hipError_t)launch_curgod(which, b, narr > 2 ? b + 2 * n : nullptr, narr > 3 ? b + 3 * n : nullptr,
                                    b + n, dofs.as<int>(), n_seg, dres.as<double>(), nullptr);
    if (e == hipSuccess) e = hipMemcpy(res, dres.p, sizeof(double) * (size_t)n_seg, hipMemcpyDeviceToHost);
  }
  d.release(); dofs.release(); dres.release();
  if (rc) return rc;
  return e == hipSuccess ? SR_OK : hip_fail(e, "sr_curgod");
}

} // extern "C"
