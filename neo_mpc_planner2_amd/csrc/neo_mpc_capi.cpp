// neo_mpc_capi.cpp -- the C-ABI of libneo_mpc.so (include/neo_mpc.h) over the gfx950 kernels.
//
// Host side of the drop-in boundary: what `NeoMpcPlanner::computeVelocityCommands`
// (src/NeoMpcPlanner.cpp:240-252) calls instead of the ROS2 service hop, and what
// `MpcOptimizationServer.__init__` (mpc_optimization_server.py:45-152) sets up.
// There is deliberately no CPU fallback: without a gfx950 device create() fails.
//
// In this order: the error setter; DeviceBuffer (device memory that frees itself, and the one-line uploads); MapFence
// (the ordering of every launch that writes or reads the device map, and the host's wait for an idle map); WorldMap (the
// world map's copy, geometry and ordering); the refusals of inflation parameters and InflationTable (K8's, K9's and K10's cached
// cost table); the handle; parameters and the term table; the shared checks; the device map (geometry, adoption, K3
// ingest); the staging of host batches by range; then the entry points -- costmaps, the solve paths of K1, K2 and the hooks,
// K4 carrots, K6 footprint gate, K7 rolling windows; a fleet's outlines (K8's and K12's one view, shape check and host
// staging), K8 fleet stamp, K9 world inflation; the scan layers -- their checks, K10's and K12 / K13's updates, the staging of an
// observation and the entry points from points, then K11: the projection, the staging of ranges and the entry points from
// ranges --; the layers read back, reset, K13's and K14's settings; K15 plan check; K16 grid planner.  A new entry point checks with the shared checks, stages with upload()
// -- an observation, ranges or outlines with the routine there is --, and launches through fence.read() or between
// fence.begin_write() and end_write(); a new kind of update is a switch of update_from_points() and from_ranges(), not a copy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "neo_mpc_device.h"
#include "solver_rules.h"

using namespace neo_mpc;

namespace {

// ---------------------------------------------------------------------------------------------- errors
thread_local std::string g_error;
thread_local int g_error_code = 0;

}  // namespace
// The one error setter (neo_mpc_rccl.cpp reports through it too)
int neo_mpc_set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
  g_error_code = code;
  return code;
}
namespace {

constexpr auto& fail = neo_mpc_set_error;

int hip_check(hipError_t e, const char* what) {
  return e == hipSuccess ? NEO_MPC_OK : fail(NEO_MPC_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e));
}
#define HIP_TRY(expr)                                 \
  do {                                                \
    if (int rc_ = hip_check((expr), #expr)) return rc_; \
  } while (0)

// ---------------------------------------------------------------------------------------------- device memory
// A device allocation that grows and is freed with its owner (the handle: hipSetDevice comes before its delete).
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }
  // (a failed re-allocation leaves the buffer empty: the old block has been let go.  A successful one never does, not even
  // for need == 0: upload() can then say "failed" with a null pointer, and a zero-sized costmap goes on to ingest()'s refusal)
  int reserve(size_t need) {
    if (ptr && need <= bytes) return NEO_MPC_OK;
    release();
    size_t cap = need + need / 4 + 256;
    HIP_TRY(hipMalloc(&ptr, cap));
    bytes = cap;
    return NEO_MPC_OK;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
  template <class T> T* as() const { return static_cast<T*>(ptr); }
  // Room for `total` bytes, then bytes [at, at + n) of it from `src` on `stream` (asynchronous) -> where they went, or
  // nullptr with the error set.
  template <class T> T* upload_range(const T* src, size_t total, size_t at, size_t n, hipStream_t stream) {
    if (reserve(total)) return nullptr;
    char* dst = as<char>() + at;
    if (hip_check(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream), "hipMemcpyAsync")) return nullptr;
    return reinterpret_cast<T*>(dst);
  }
  template <class T> T* upload(const T* src, size_t n, hipStream_t stream) { return upload_range(src, n, 0, n, stream); }
  // ... and back: bytes [at, at + n) to `dst` on `stream` (asynchronous)
  int download_range(void* dst, size_t at, size_t n, hipStream_t stream) const {
    return hip_check(hipMemcpyAsync(dst, as<char>() + at, n, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
  }
  // The whole of `src` with a blocking copy: it is free when this returns
  template <class T> T* upload(const T* src, size_t n) {
    if (reserve(n) || hip_check(hipMemcpy(ptr, src, n, hipMemcpyHostToDevice), "hipMemcpy")) return nullptr;
    return as<T>();
  }
};

// ---------------------------------------------------------------------------------------------- the map fence
// The event recorded behind the last write of a buffer, the stream it went to, and the waits for it: on a stream (skipped on
// that stream itself: in order anyway) or on the host.  What MapFence and WorldMap both keep of their writer.
struct WriteEvent {
  hipEvent_t ready = nullptr;
  hipStream_t ready_stream = nullptr;
  int wait_writer(hipStream_t st) {
    if (ready && ready_stream != st) HIP_TRY(hipStreamWaitEvent(st, ready, 0));
    return NEO_MPC_OK;
  }
  int wait_writer_host() {
    if (ready) HIP_TRY(hipEventSynchronize(ready));
    return NEO_MPC_OK;
  }
  void destroy() { if (ready) (void)hipEventDestroy(ready); }
};

// Stream ordering around the device map (map_buf).  A WRITE -- ingest, roll, stamp: the kernels that rewrite the maps in
// place -- runs behind the previous write and behind every launch still reading the maps, whatever stream it went to, and
// records `ready` on its stream.  A READ -- every solve / postprocess / objective / gate launch -- waits for `ready` on its
// own stream and records the in-use event OF ITS STREAM (one per distinct stream the caller has used), which the next
// write waits for.  (Waits on the stream an event was recorded on are skipped: in order anyway.)
struct MapFence : WriteEvent {
  static constexpr size_t kMaxUsers = 64;   // distinct streams with a launch in flight between two writes
  struct User { hipStream_t stream; hipEvent_t done; bool pending; };
  std::vector<User> users;

  int begin_write(hipStream_t st) {
    if (!ready) HIP_TRY(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    else if (ready_stream != st) HIP_TRY(hipStreamWaitEvent(st, ready, 0));   // (two writes must not overlap in map_buf)
    for (auto& u : users)
      if (u.pending && u.stream != st) HIP_TRY(hipStreamWaitEvent(st, u.done, 0));
    return NEO_MPC_OK;
  }
  // (the readers begin_write queued its waits for are covered by `ready` from here on, and only from here on: a write whose
  // launch failed leaves them pending)
  int end_write(hipStream_t st) {
    HIP_TRY(hipEventRecord(ready, st));
    ready_stream = st;
    for (auto& u : users) u.pending = false;
    return NEO_MPC_OK;
  }
  // `launch` enqueues one kernel that reads the maps on `stream`
  template <class Launch> int read(void* stream, Launch&& launch) {
    hipStream_t st = (hipStream_t)stream;
    int rc = wait_writer(st);
    if (rc) return rc;
    launch();
    HIP_TRY(hipGetLastError());
    return release(st);
  }
  // The host's wait for a map nobody is using: before the term table or the pool's origins are rewritten (blocking copies
  // on the null stream, which do not order against the non-blocking streams batches are in flight on) every launch that
  // may still read them has to have ENDED.  Those are the pending readers -- and the readers a write has already cleared:
  // begin_write only queued a wait for them on its stream, so they may still be running, but end_write recorded `ready` on
  // that stream behind those waits, and it ends after every one of them.  (The device map itself is ordered by the stream waits
  // above; these two small tables change on reconfiguration / pool re-centring only, so a host-side wait is cheap.)
  int wait_idle() {
    for (auto& u : users)
      if (u.pending) HIP_TRY(hipEventSynchronize(u.done));
    return wait_writer_host();
  }
  void destroy() {
    WriteEvent::destroy();
    for (auto& u : users) (void)hipEventDestroy(u.done);
  }

 private:
  // one event per distinct stream, re-recorded by that stream's latest launch
  int release(hipStream_t st) {
    User* slot = nullptr;
    for (auto& u : users) if (u.stream == st) { slot = &u; break; }
    if (!slot) {
      if (users.size() >= kMaxUsers) {
        // more streams than slots: the oldest slot's launch is waited for here and the slot re-used
        slot = &users.front();
        if (slot->pending) HIP_TRY(hipEventSynchronize(slot->done));
        slot->stream = st;
      } else {
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        users.push_back({st, ev, false});
        slot = &users.back();
      }
    }
    HIP_TRY(hipEventRecord(slot->done, st));
    slot->pending = true;
    return NEO_MPC_OK;
  }
};

// ---------------------------------------------------------------------------------------------- the world map
// K7, K9.  The handle's own device copy of the world map the rolling windows are cut from, and its geometry.  Every rewrite
// -- a new copy, the inflation in place -- runs behind the last roll, which reads the copy that is about to change, and
// behind the previous rewrite.  The last roll is the fence's last write or lies behind it -- every write runs behind the one
// before -- so the wait is for that write whatever it was: `rolled` says nothing here, an ingest enqueued behind a roll that
// has not started clears it.  On `st` for the device variants, on the host for the synchronous ones.  Every rewrite ends
// with `ready` recorded: a roll on another stream, the next rewrite and the host's read wait for it.
struct WorldMap : WriteEvent {
  DeviceBuffer buf;
  bool has = false;
  int32_t size_x = 0, size_y = 0;
  double resolution = 0.0, origin_x = 0.0, origin_y = 0.0;
  int begin_write(MapFence& fence, bool on_stream, hipStream_t st) {
    if (int rc = on_stream ? fence.wait_writer(st) : fence.wait_writer_host()) return rc;
    return on_stream ? wait_writer(st) : wait_writer_host();
  }
  int end_write(hipStream_t st) {
    if (!ready) HIP_TRY(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ready, st));
    ready_stream = st;
    return NEO_MPC_OK;
  }
};

// ---------------------------------------------------------------------------------------------- inflation parameters
// K8, K9.  The cost table of the contract (neo_mpc_stamp_batch): nav2's InflationLayer::computeCost by squared cell distance.
void stamp_costs(double res, double ins, double csf, int reach, uint8_t* table) {
  table[0] = 254;
  for (int n = 1; n <= reach * reach; ++n) {
    const double dist = std::sqrt((double)n) * res;
    if (dist <= ins) table[n] = 253;
    else {
      const double factor = std::exp(-csf * (dist - ins));
      table[n] = (uint8_t)(252.0 * factor);
    }
  }
}
// The refusals of inflation parameters, once: the radii alone (what an entry point refuses before it looks at its map) ...
int check_inflation_radii(double ins, double infl, double csf) {
  if (std::isfinite(ins) && std::isfinite(infl) && std::isfinite(csf) && ins >= 0.0 && infl >= 0.0 && csf >= 0.0) return NEO_MPC_OK;
  return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "inscribed_radius %g, inflation_radius %g and cost_scaling_factor %g must be finite and not negative", ins, infl, csf);
}
// ... and all of them at a resolution (`whose` map's: "" or "the world map's ") -> R = ceil(inflation_radius / res) in
// `reach` (if asked for), refused beyond NEO_MPC_MAX_INFLATION_CELLS (compared in float64, before the conversion)
int inflation_reach(double res, double ins, double infl, double csf, const char* whose, int* reach) {
  if (int rc = check_inflation_radii(ins, infl, csf)) return rc;
  const double r = std::ceil(infl / res);
  if (!(r <= (double)NEO_MPC_MAX_INFLATION_CELLS))
    return fail(NEO_MPC_ERR_UNSUPPORTED, "inflation_radius %g at %sresolution %g is more than %d cells", infl, whose, res, NEO_MPC_MAX_INFLATION_CELLS);
  if (reach) *reach = (int)r;
  return NEO_MPC_OK;
}

// The table on the device and the parameters it was built for.  A call with the parameters of the previous one -- the stamp
// of every tick, the inflation behind every new world map -- finds it in place: nothing is built, allocated or copied, so
// the call can be captured in a graph.  build(): for parameters inflation_reach() has passed;
// `readers`: the writer whose launches read the table -- those in flight read the old one to their end.
struct InflationTable {
  DeviceBuffer buf;
  bool valid = false;
  double key[4] = {0.0, 0.0, 0.0, 0.0};   // resolution, inscribed_radius, inflation_radius, cost_scaling_factor
  int32_t reach = 0;
  int build(double res, double ins, double infl, double csf, WriteEvent& readers) {
    const double now[4] = {res, ins, infl, csf};
    if (valid && std::memcmp(now, key, sizeof(key)) == 0) return NEO_MPC_OK;
    const int r = (int)std::ceil(infl / res);   // (inflation_reach() has passed these parameters: R <= NEO_MPC_MAX_INFLATION_CELLS)
    int rc;
    std::vector<uint8_t> table((size_t)r * r + 1);
    stamp_costs(res, ins, csf, r, table.data());
    if ((rc = readers.wait_writer_host())) return rc;
    valid = false;
    // (the largest table, once: a change of parameters never re-allocates)
    if ((rc = buf.reserve((size_t)NEO_MPC_MAX_INFLATION_CELLS * NEO_MPC_MAX_INFLATION_CELLS + 1))) return rc;
    if (!buf.upload(table.data(), table.size())) return NEO_MPC_ERR_DEVICE;
    std::memcpy(key, now, sizeof(key));
    reach = r;
    valid = true;
    return NEO_MPC_OK;
  }
};

// ---------------------------------------------------------------------------------------------- the scan layers
// K10.  An obstacle layer per window of the pool, rows padded to 64 bytes: `layer` holds the layers between updates, `work`
// those of the update in flight, `origins` the layers' origins; a cost table of their own; and what the layers were made
// for -- an update that meets another geometry or unknown_value resets them.
struct ScanLayers {
  InflationTable table;
  DeviceBuffer layer, work, origins;
  bool valid = false;
  int32_t size_x = 0, size_y = 0, count = 0;
  double resolution = 0.0;
  uint32_t unknown = 0;
  DeviceBuffer points, point_counts, sensors;   // (the host variant's staging)
  int pitch() const { return (size_x + 63) & ~63; }
  size_t stride() const { return (size_t)pitch() * (size_t)size_y; }
  bool matches(const DevMap& m, uint32_t u) const {
    return valid && size_x == m.size_x && size_y == m.size_y && count == m.pool_count && resolution == m.resolution && unknown == u;
  }
  // A reset: the pool's geometry, nobody's until adopt(); re-allocated only where that asks for more (which synchronises)
  int resize(const DevMap& m, uint32_t unknown_value) {
    valid = false;
    size_x = m.size_x; size_y = m.size_y; count = m.pool_count; resolution = m.resolution; unknown = unknown_value;
    if (int rc = layer.reserve(stride() * (size_t)count)) return rc;
    if (int rc = work.reserve(stride() * (size_t)count)) return rc;
    return origins.reserve((size_t)count * 16);
  }
  void adopt() { valid = true; }   // behind the update's end_write: its launches are enqueued
};

// K12.  The fleet's shared obstacle layer on the world map's lattice: `layer` persists between updates, `live` is the world
// map with the layer merged in and inflated -- what the roll reads while `live_valid` --, both WSX bytes a row; a cost table of
// their own at the world's resolution; and what the layer was made for -- an update that meets another geometry or
// unknown_value resets it.  Ordered by the world map's own event (WorldMap): an update is a rewrite of what the roll reads.
// K13, the speckle filter: its setting -- configuration, which outlives resets and world maps --, D, the layer as the
// composition of the last update read it, allocated only while the filter is on, and whether that update filtered.
// K14, decay: its setting -- configuration too --, `stamp`, a word per cell, and `clock`, one word, both allocated by the first
// update with decay on, and whether the last update ran with it: the stamps then go with the layer's marks.
struct WorldScanLayer {
  InflationTable table;
  DeviceBuffer layer, live;
  DeviceBuffer denoised;
  DeviceBuffer stamp, clock;
  uint32_t group = 0, connectivity = 8;   // neo_mpc_set_world_scan_denoise: G (0: off) and 4 or 8
  uint32_t max_age = 0;      // neo_mpc_set_world_scan_decay: A, scan updates (0: off)
  bool filtered = false;     // the last update wrote D
  bool decaying = false;     // the last update ran with decay on
  bool valid = false;        // the layer holds what the updates since the last reset put there
  bool live_valid = false;   // `live` is the current world map with the layer in it
  int32_t size_x = 0, size_y = 0;
  double resolution = 0.0, origin_x = 0.0, origin_y = 0.0;
  uint32_t unknown = 0;
  // (the host variants' staging of the clear record, stage_outlines().  Apart from the handle's verts / poses / problems, which
  // K6 and K8 stage into: K12's host variant from ranges has the handle's `poses` in use for the laser poses)
  DeviceBuffer verts, poses, problems;
  size_t bytes() const { return (size_t)size_x * (size_t)size_y; }
  bool matches(const WorldMap& w, uint32_t u) const {
    return valid && size_x == w.size_x && size_y == w.size_y && resolution == w.resolution && origin_x == w.origin_x &&
           origin_y == w.origin_y && unknown == u;
  }
  // A reset: the world's geometry; re-allocated only where that asks for more (which synchronises)
  int resize(const WorldMap& w, uint32_t unknown_value) {
    valid = false; live_valid = false;
    size_x = w.size_x; size_y = w.size_y; resolution = w.resolution; origin_x = w.origin_x; origin_y = w.origin_y;
    unknown = unknown_value;
    if (int rc = layer.reserve(bytes())) return rc;
    return live.reserve(bytes());
  }
  // D: a no-op from the second update with this geometry and setting on
  int reserve_denoised() { return group >= 2 ? denoised.reserve(bytes()) : NEO_MPC_OK; }
  // `stamp` and `clock`: no-ops from the second update with this geometry and decay on.  The clock starts at 0 (a blocking
  // fill); a stamp is read only under a mark, and a layer that has just been made or reset holds none
  int reserve_decay() {
    if (max_age == 0) return NEO_MPC_OK;
    if (int rc = stamp.reserve(bytes() * sizeof(uint32_t))) return rc;
    if (clock.ptr) return NEO_MPC_OK;
    if (int rc = clock.reserve(sizeof(uint32_t))) return rc;
    HIP_TRY(hipMemset(clock.ptr, 0, sizeof(uint32_t)));
    return NEO_MPC_OK;
  }
};

// K11.  The beam table of one scanner (the contract: neo_mpc_laser_batch, step 4), with libm
void laser_beam_table(const neo_mpc_scanner& sc, uint32_t beams, double* table) {
#pragma clang fp contract(off)
  for (uint32_t i = 0; i < beams; ++i) {
    const double a = sc.mount_yaw + (sc.angle_min + (double)i * sc.angle_increment);
    table[2 * (size_t)i] = std::cos(a);
    table[2 * (size_t)i + 1] = std::sin(a);
  }
}

// K11.  The beam tables on the device and the scanners they were built for, the handle's own points and origins -- what an
// update without points_out / origins_out projects into -- and the host variants' staging of the ranges.  A call with the
// scanners, beams and count of the previous one finds all of it in place: nothing is built, allocated or copied, so the call
// can be captured in a graph.
struct LaserProjection {
  DeviceBuffer table, points, origins;
  DeviceBuffer ranges;                    // (the host variants' staging)
  std::vector<unsigned char> key;         // the scanners' bytes, then `beams`
  bool valid = false;
  // for scanners check_scanner() has passed.  The launches in flight, on whatever stream, read the old tables to their end:
  // a change of scanners is configuration, and waits for the device.
  int build(const neo_mpc_scanner* scanners, uint32_t sources, uint32_t beams) {
    std::vector<unsigned char> now(sources * sizeof(neo_mpc_scanner) + sizeof(beams));
    std::memcpy(now.data(), scanners, sources * sizeof(neo_mpc_scanner));
    std::memcpy(now.data() + sources * sizeof(neo_mpc_scanner), &beams, sizeof(beams));
    if (valid && now == key) return NEO_MPC_OK;
    std::vector<double> host((size_t)sources * beams * 2);
    for (uint32_t s = 0; s < sources; ++s) laser_beam_table(scanners[s], beams, host.data() + (size_t)s * beams * 2);
    HIP_TRY(hipDeviceSynchronize());
    valid = false;
    // (the largest table, once: a change of scanners never re-allocates)
    if (int rc = table.reserve((size_t)NEO_MPC_MAX_SCAN_POINTS * 16)) return rc;
    if (!table.upload(host.data(), host.size() * 8)) return NEO_MPC_ERR_DEVICE;
    key.swap(now);
    valid = true;
    return NEO_MPC_OK;
  }
  // the handle's own out buffers: no-ops from the second call with this shape on (a re-allocation frees, which synchronises)
  int reserve_out(size_t count, uint32_t sources, uint32_t beams, bool want_points, bool want_origins) {
    if (want_points) if (int rc = points.reserve(count * sources * beams * 16)) return rc;
    if (want_origins) if (int rc = origins.reserve(count * sources * 16)) return rc;
    return NEO_MPC_OK;
  }
};

}  // namespace

// (hidden: its destructor, no longer trivial, is no export)
struct __attribute__((visibility("hidden"))) neo_mpc_handle {
  int device = 0;
  neo_mpc_params params{};
  DevParams dp{};
  LdsLayout lds{};
  // the environment's A/B switches, read once by neo_mpc_create (include/neo_mpc.h)
  LaunchTuning tuning;
  bool no_chunks = false;     // NEO_MPC_NO_CHUNKS: large staged host batches go through in one piece
  int auto_host_path = NEO_MPC_HOST_PATH_ZEROCOPY;   // what NEO_MPC_HOST_PATH_AUTO means (NEO_MPC_HOST_PATH)
  // the device map: one costmap or a pool (map_buf; raw_buf and origins_buf: the host variants' cells and origins), the
  // term table of the costmap weight, and their ordering
  DevMap map{};
  bool has_map = false;
  bool rolled = false;                      // the device map was written by a roll (its buffers and constants are in place)
  DeviceBuffer map_buf, raw_buf, term_buf, origins_buf;
  MapFence fence;
  // staging of host batches: the records of a batch, and what the host variants of K4 / K6 / K7 / K8 share -- a fleet's
  // [count][3] poses and its footprint or polygon vertices.  (Every host variant has finished with its staging when it
  // returns -- a blocking copy or a synchronisation behind its kernel -- so one buffer serves them all.)
  DeviceBuffer problems, states, warm, commands, solution, path, vel, footprints, success, u, cost;
  DeviceBuffer poses, verts;
  int host_path = NEO_MPC_HOST_PATH_AUTO;   // neo_mpc_set_host_path
  // latency path of neo_mpc_solve_batch (small host batches, the plugin's count = 1): one pinned
  // staging block and one device arena, so a tick is one H2D, K1, one D2H and one synchronisation
  void* pin = nullptr;
  DeviceBuffer arena;
  hipStream_t chunk_streams[2] = {nullptr, nullptr};   // staged host batches of >= kChunkedMinCount instances: copy / solve pipeline
  // neo_mpc_solve_batch_begin / _wait: page-locked batches in flight, each on a stream of its own
  struct InFlight { hipStream_t stream = nullptr; hipEvent_t done = nullptr; bool busy = false; };
  InFlight in_flight[NEO_MPC_MAX_BATCHES_IN_FLIGHT];
  DeviceBuffer order_buf;     // dispatch order of device batches (neo_mpc_balance_dispatch_device)
  DeviceBuffer load_buf;      // ... and the exponential average of the iteration counts it is sorted by
  size_t order_count = 0;     // ... armed for batches of this many instances; 0: launch order
  // K4 neo_mpc_select_carrots (its robot poses: poses) and K6 neo_mpc_footprint_gate (its polygon: verts; fp_costs: both)
  DeviceBuffer plan_poses, plan_offsets, fp_costs, slow_down, carrots;
  DeviceBuffer gate_indices, gate_polygons_out;
  // K7 neo_mpc_set_world_map / neo_mpc_roll_costmap_pool: the world map and the fill's index tables
  WorldMap world;
  DeviceBuffer roll_tables;
  // K8 neo_mpc_stamp_fleet: the cost table at the windows' resolution, the oriented polygons and their bounding boxes
  InflationTable stamp_table;
  DeviceBuffer stamp_polys, stamp_boxes;
  // K9 neo_mpc_inflate_world_map: its own cost table -- the world's resolution need not be the windows'
  InflationTable world_table;
  ScanLayers scan;   // K10 neo_mpc_update_scan_layer
  LaserProjection laser;   // K11 neo_mpc_project_laser, neo_mpc_update_scan_layer_from_ranges
  WorldScanLayer world_scan;   // K12 neo_mpc_update_world_scan_layer
  DeviceBuffer plan_checks;    // K15 neo_mpc_check_plans: its results (its plans: K4's plan_poses / plan_offsets; poses, verts)
};
constexpr size_t kLatencyPathMaxCount = 64;
constexpr size_t kChunkedMinCount = 65536;   // staged host batches from here on go through in kChunks pieces on two streams
                                             // (measured: pageable 32 768 instances 24.0 M solves/s in pieces against 28.6 M in one,
                                             // 65 536: 38.9 / 31.6, 131 072: 42.6 / 32.5, 262 144: 45.3 / 33.2)
constexpr size_t kChunks = 4;
constexpr size_t kLatencyPathBytes = kLatencyPathMaxCount * (sizeof(neo_mpc_problem) + sizeof(neo_mpc_state) +
                                                            sizeof(neo_mpc_command) + 24 +
                                                            3 * 3 * NEO_MPC_MAX_CONTROL_STEPS * 8);

namespace {

int validate(const neo_mpc_params& p, bool live_handle) {
  if (p.control_steps < 1 || p.control_steps > NEO_MPC_MAX_CONTROL_STEPS)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "control_steps %d outside [1, %d]", p.control_steps,
                NEO_MPC_MAX_CONTROL_STEPS);
  if (!(p.prediction_horizon > 0.0)) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "prediction_horizon must be > 0");
  if (!(p.min_vel_x <= p.max_vel_x) || !(p.min_vel_y <= p.max_vel_y) || !(p.min_vel_theta <= p.max_vel_theta))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "velocity bounds: min > max");  // SciPy raises here too
  if (!(p.max_vel_trans > 0.0)) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "max_vel_trans must be > 0");
  // box ∩ disc must be non-empty: closest box point to the origin inside the disc
  double nx = std::fmin(std::fmax(0.0, p.min_vel_x), p.max_vel_x);
  double ny = std::fmin(std::fmax(0.0, p.min_vel_y), p.max_vel_y);
  if (nx * nx + ny * ny > p.max_vel_trans * p.max_vel_trans)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "velocity box does not intersect the max_vel_trans disc");
  if (p.method < 0 || p.method > NEO_MPC_METHOD_RICCATI) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown method %d", p.method);
  if (p.method == NEO_MPC_METHOD_NEWTON && p.control_steps > NEO_MPC_NEWTON_MAX_CONTROL_STEPS)
    return fail(NEO_MPC_ERR_UNSUPPORTED, "NEO_MPC_METHOD_NEWTON is built for control_steps <= 8 only (got %d)",
                p.control_steps);
  if (p.lbfgs_memory > NEO_MPC_MAX_LBFGS_MEMORY)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "lbfgs_memory > %d", NEO_MPC_MAX_LBFGS_MEMORY);
  if (p.compat_flags & ~NEO_MPC_COMPAT_ALL)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown compat_flags bits 0x%x (known: 0x%x)", p.compat_flags & ~NEO_MPC_COMPAT_ALL,
                NEO_MPC_COMPAT_ALL);
  // no selectable configuration is knowingly worse than the reference: the L-BFGS and the dense Newton direction have no
  // wall model for costmap steps, and forced onto a heavy costmap weight they end above SLSQP on a few percent of the
  // costmap cases (G8 "turn": up to 1.0 at control_steps 8; G9: 2 of 48 up to 4e-3) -- AUTO never sends them there
  // (neo_mpc_create refuses; a live handle reconfigured across the threshold runs the stage-wise direction instead --
  // cb_params cannot fail in the reference, and a controller must not lose its solver to a weight change: solver_rules.h)
  if (!live_handle && (p.method == NEO_MPC_METHOD_LBFGS || p.method == NEO_MPC_METHOD_NEWTON) && p.w_costmap > 0.25 * p.w_trans)
    return fail(NEO_MPC_ERR_UNSUPPORTED, "method %d has no wall model for costmap steps: not offered with w_costmap > w_trans / 4 "
                "(%g > %g); use NEO_MPC_METHOD_AUTO or NEO_MPC_METHOD_RICCATI", p.method, p.w_costmap, 0.25 * p.w_trans);
  return NEO_MPC_OK;
}

int occupancy(int raw) {  // nav2 Costmap2DPublisher translation (build's costmap contract)
  if (raw == 0) return 0;
  if (raw == 253) return 99;
  if (raw == 254) return 100;
  if (raw == 255) return -1;
  return 1 + (97 * (raw - 1)) / 251;
}

void derive(neo_mpc_handle* h) {
  const neo_mpc_params& p = h->params;
  DevParams& d = h->dp;
  const int n = p.control_steps;
  d.n = n;
  d.dt = p.prediction_horizon / n;  // py:137
  d.wt_n = p.w_trans / n;
  d.wo_n = p.w_orient / n;
  d.wc_n = p.w_control / n;
  d.wterm_o = p.w_terminal * p.w_orient;
  d.wterm_t = p.w_terminal * p.w_trans;
  d.w_footprint = p.w_footprint;
  d.lo[0] = p.min_vel_x; d.hi[0] = p.max_vel_x;
  d.lo[1] = p.min_vel_y; d.hi[1] = p.max_vel_y;
  d.lo[2] = p.min_vel_theta; d.hi[2] = p.max_vel_theta;
  d.r = p.max_vel_trans;
  d.acc[0] = p.acc_x_limit; d.acc[1] = p.acc_y_limit; d.acc[2] = p.acc_theta_limit;
  d.low_pass_gain = p.low_pass_gain;
  // every tolerance of the search comes out of solver_rules.h -- the one rule book the device code and the CPU mirror
  // (test infrastructure) share; all of them derive from opt_tolerance
  neo_rules r;
  neo_rules_derive(&p, &r);
  d.xtol = r.xtol;
  d.kink_radius = r.kink_radius;
  {
    neo_rules rs;   // (the rules of the instances the routed kernel sends to the stage-wise direction)
    neo_rules_derive_as(&p, NEO_DIRECTION_STAGEWISE, &rs);
    d.kink_radius_stagewise = rs.kink_radius;
  }
  d.stall_step = r.stall_step;
  d.hop_min_drop = r.hop_min_drop;
  d.hop_range = h->has_map ? neo_rules_hop_range(d.dt, h->map.resolution) : NEO_RULE_HOP_DIST;
  d.scan_resume_gain = r.scan_resume_gain;
  d.scan_reach = h->has_map ? neo_rules_reach_cells(&p, h->map.resolution) : 0;
  d.max_it = r.max_iterations;
  d.mem = r.lbfgs_memory;
  d.compat = (p.compat_flags & NEO_MPC_COMPAT_ODOM_YAW_GOAL_W) |
             ((p.compat_flags & NEO_MPC_COMPAT_REFERENCE_START) ? kCompatNoUnshift : 0);
  d.disc_in_box = (p.min_vel_x <= -p.max_vel_trans && p.max_vel_x >= p.max_vel_trans &&
                   p.min_vel_y <= -p.max_vel_trans && p.max_vel_y >= p.max_vel_trans) ? 1 : 0;
  d.tame = (d.disc_in_box && fmax(fabs(p.min_vel_theta), fabs(p.max_vel_theta)) * p.prediction_horizon <= 0.78) ? 1 : 0;
  // search direction: AUTO = the register-resident dense Newton kernel at control_steps 3 (the headline
  // specialisation), the stage-wise (Riccati) Newton sweep of the run-time-sized kernel otherwise -- and at 3 too
  // when the costmap weight is heavy (w_costmap > w_trans / 4; the README's is w_trans / 16): cost steps are then
  // walls the search has to slide along, and the wall model lives in the stage-wise direction (costmap.h).  Against
  // the reference's SLSQP solves at w_costmap = 0.3 (G8 "turn") the dense direction ends 3e-3 and 9e-3 above
  // SLSQP's value in 2 of 24 cases, the stage-wise one in none.
  d.newton = r.direction;
  // (round 6) AUTO at control_steps 3: direction by neighbourhood -- dense where the reach tile is all free, stage-wise
  // elsewhere (solver_rules.h neo_rules_routes_by_neighbourhood; method = NEO_MPC_METHOD_NEWTON is the dense direction for
  // every instance: round 5's AUTO, the A/B partner)
  d.routed = (neo_rules_routes_by_neighbourhood(&p) && r.direction == NEO_DIRECTION_DENSE) ? 1 : 0;
  d.early_tol = r.xtol;
  d.final_tol = r.final_tol;
  d.ftol = r.ftol;
  d.wtol = r.wtol;
  d.wtol_late = r.wtol_late;
  d.btol_map = r.btol_map;
  d.btol_free = r.btol_free;

  // LDS carve-up (shared with the kernel specialisations) + reach tile geometry
  LdsLayout& l = h->lds;
  // the control_steps == 3 specialisations carve LDS at compile time with 4 pair slots; the host
  // must reserve exactly that layout whenever launch_solve() will pick them
  const bool specialised = n == 3 && (d.newton == 1 || (d.newton == 0 && d.mem == 4));
  l = make_lds_layout(n, specialised ? 4 : (d.newton ? 0 : d.mem), d.newton == 2, !d.disc_in_box);
  const int off = l.tile;
  l.tile_w = 0; l.tile_h = 0; l.reach = 0;
  if (h->has_map) {
    const int R = neo_rules_reach_cells(&p, h->map.resolution);   // (solver_rules.h: the cell scan's radius too)
    const int w = neo_rules_tile_width(R);   // (0: no tile -- a reach beyond 60 cells)
    if (w) { l.reach = R; l.tile_w = w; l.tile_h = 2 * R + 1; }
  }
  l.total_bytes = off * 8 + l.tile_w * l.tile_h;
  l.total_bytes = (l.total_bytes + 15) & ~15;
}

int upload_term_table(neo_mpc_handle* h) {
  double table[256];
  const neo_mpc_params& p = h->params;
  const int n = p.control_steps;
  for (int raw = 0; raw < 256; ++raw) {
    const double c = (double)occupancy(raw) / 100.0;  // getCost contract
    const double cc = c * c;                           // py:247
    table[raw] = (c == 1.0) ? cc * 1000 / n : p.w_costmap * cc / n;  // py:257-260
  }
  int rc = h->fence.wait_idle();   // (a batch in flight reads the old table to its end)
  if (rc) return rc;
  return h->term_buf.upload(table, sizeof(table)) ? NEO_MPC_OK : NEO_MPC_ERR_DEVICE;
}

int apply_params(neo_mpc_handle* h, const neo_mpc_params* params, bool live_handle) {
  int rc = validate(*params, live_handle);
  if (rc) return rc;
  h->params = *params;
  derive(h);
  return upload_term_table(h);
}

// ---------------------------------------------------------------------------------------------- shared checks
int check_count(size_t count, size_t most = 0x7fffffffull) {
  return count > most ? fail(NEO_MPC_ERR_INVALID_ARGUMENT, "count too large") : NEO_MPC_OK;
}

int check_pool_count(uint32_t count) {
  if (count == 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "bad costmap count %u", count);
  if (count > NEO_MPC_MAX_POOL_MAPS)   // K3 takes the map index from the grid's y coordinate
    return fail(NEO_MPC_ERR_UNSUPPORTED, "costmap pool of %u maps: at most %u per call", count, NEO_MPC_MAX_POOL_MAPS);
  return NEO_MPC_OK;
}

int check_footprint_shape(uint32_t points, uint32_t per_robot) {
  if (points < 3 || points > NEO_MPC_MAX_FOOTPRINT_POINTS)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "footprint_points %u outside [3, %d]", points, NEO_MPC_MAX_FOOTPRINT_POINTS);
  if (per_robot > 1) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "per_robot_footprints must be 0 or 1 (got %u)", per_robot);
  return NEO_MPC_OK;
}

// The value checks of the host variants (the device variants take values as they come).  `polygons` polygons of `np` vertices:
int check_vertices_finite(const double* v, size_t polygons, size_t np, const char* vertex, const char* polygon) {
  for (size_t k = 0; k < polygons * np * 2; ++k)
    if (!std::isfinite(v[k]))
      return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "%s %zu of %s %zu is not finite", vertex, (k / 2) % np, polygon, k / (2 * np));
  return NEO_MPC_OK;
}

// ... and the poses a footprint is placed at: poses[i], else the pose of problems[i].  `more(i)`: what else a caller looks at
// robot by robot, behind robot i's pose
inline int nothing_more(size_t) { return NEO_MPC_OK; }
template <class More = int (*)(size_t)>
int check_poses_finite(const double* poses, const neo_mpc_problem* problems, size_t n, More&& more = nothing_more) {
  for (size_t i = 0; i < n; ++i) {
    bool finite = true;
    if (poses) for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(poses[3 * i + k]);
    else {
      for (int k = 0; k < 2; ++k) finite = finite && std::isfinite(problems[i].cur_xy[k]);
      for (int k = 0; k < 4; ++k) finite = finite && std::isfinite(problems[i].cur_q[k]);
    }
    if (!finite) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "the pose of robot %zu is not finite", i);
    if (int rc = more(i)) return rc;
  }
  return NEO_MPC_OK;
}

// ---------------------------------------------------------------------------------------------- the device map
// A map of sx x sy cells as it lies in map_buf: `border` cells around it, rows pitched to 128 bytes.
struct PaddedMap {
  uint32_t sx, sy;
  int border, pitch, rows;
  size_t stride;   // bytes from one map of a pool to the next
  PaddedMap(uint32_t sx_, uint32_t sy_, int border_)
      : sx(sx_), sy(sy_), border(border_), pitch((int)((sx_ + 2 * border_ + 127) & ~127u)), rows((int)sy_ + 2 * border_),
        stride((size_t)pitch * rows) {}
  // K3 and K7 index the 16-byte chunks of one map with 32 bits
  int check(const char* what) const {
    if (stride / 16 < (1ull << 31)) return NEO_MPC_OK;
    return fail(NEO_MPC_ERR_UNSUPPORTED, "%s %ux%u is too large (over 32 GiB padded)", what, sx, sy);
  }
};

// map_buf holds `maps` such maps from here on (d_origins == nullptr: the single map with origin (ox, oy))
void adopt_map(neo_mpc_handle* h, const PaddedMap& g, uint32_t maps, double res, double ox, double oy, const double* d_origins,
               bool rolled) {
  h->map.cells = h->map_buf.as<const uint8_t>() + (size_t)g.border * g.pitch + g.border;
  h->map.size_x = (int)g.sx; h->map.size_y = (int)g.sy; h->map.pitch = g.pitch;
  h->map.resolution = res; h->map.inv_resolution = 1.0 / res;
  h->map.origin_x = ox; h->map.origin_y = oy;
  h->map.pool_count = d_origins ? (int)maps : 0;
  h->map.border = g.border;
  h->map.pool_stride = (int64_t)g.stride;
  h->map.pool_origins = d_origins;
  h->has_map = true;
  h->rolled = rolled;
  derive(h);
}

// `maps` raw costmaps back to back in device memory -> bordered, pitched device maps (K3).
// d_origins == nullptr: a single map with origin (ox, oy); else a pool whose origins stay where they are.
int ingest(neo_mpc_handle* h, const uint8_t* d_cells, uint32_t maps, uint32_t sx, uint32_t sy, double res, double ox,
           double oy, const double* d_origins, void* stream) {
  if (!d_cells || maps == 0 || sx == 0 || sy == 0 || sx > (1u << 20) || sy > (1u << 20) || !(res > 0.0))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "bad costmap geometry %ux%u x%u res %g", sx, sy, maps, res);
  const PaddedMap g(sx, sy, d_origins ? kPoolBorder : kMapBorder);
  int rc = g.check("costmap");
  if (rc) return rc;
  if ((rc = h->map_buf.reserve(g.stride * maps))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = h->fence.begin_write(st))) return rc;
  IngestArgs a;
  a.src = d_cells;
  a.dst = h->map_buf.as<uint8_t>();
  a.size_x = (int)sx; a.size_y = (int)sy; a.pitch = g.pitch; a.rows = g.rows;
  a.maps = (int)maps; a.border = g.border; a.dst_stride = (int64_t)g.stride;
  launch_ingest(a, h->tuning, stream);
  HIP_TRY(hipGetLastError());
  if ((rc = h->fence.end_write(st))) return rc;
  adopt_map(h, g, maps, res, ox, oy, d_origins, false);
  return NEO_MPC_OK;
}

int fill_args(neo_mpc_handle* h, const neo_mpc_batch* b, SolveArgs& a) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (!b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null batch");
  if (!h->has_map) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_costmap has not been called");
  if (b->count > 0 && (!b->problems || !b->states || !b->warm_start || !b->commands))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "problems/states/warm_start/commands must not be null");
  if (int rc = check_count(b->count)) return rc;
  if (b->footprints && b->footprint_points > NEO_MPC_MAX_FOOTPRINT_POINTS)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "footprint_points > %d", NEO_MPC_MAX_FOOTPRINT_POINTS);
  std::memset(&a, 0, sizeof(a));
  a.problems = b->problems; a.states = b->states; a.warm = b->warm_start; a.commands = b->commands;
  a.solution = b->solution; a.path = b->predicted_path; a.velocities = b->velocities;
  a.states_out = b->states; a.warm_out = b->warm_start;
  a.footprints = b->footprint_points ? b->footprints : nullptr;
  a.footprint_points = b->footprints ? b->footprint_points : 0;
  a.count = (uint32_t)b->count;
  a.term_table = h->term_buf.as<const double>();
  a.p = h->dp; a.map = h->map; a.lds = h->lds;
  return NEO_MPC_OK;
}

// K1 with `a` on `stream`, in its place between the map's writes
int solve_on(neo_mpc_handle* h, const SolveArgs& a, void* stream) {
  return h->fence.read(stream, [&] { launch_solve(a, h->tuning, stream); });
}

// ---------------------------------------------------------------------------------------------- staging of host batches
// Host batches go up and come back by range: records [off, off + m) of the batch `b`, to and from their place in the handle's
// staging buffers (sized for the whole batch), queued on `st`.  A staged batch is the range [0, count) on the null stream,
// a chunked one kChunks ranges on two streams.  Every copy is asynchronous: the caller leaves no way out while one may
// still be reading or writing the host arrays.
//
// The request / state / warm-start records -> d.problems, d.states, d.warm_start
int stage_records(neo_mpc_handle* h, const neo_mpc_batch* b, size_t off, size_t m, hipStream_t st, neo_mpc_batch& d) {
  const size_t n = b->count, nv = 3 * (size_t)h->params.control_steps;
  const size_t prob = sizeof(neo_mpc_problem), state = sizeof(neo_mpc_state), row = nv * 8;
  d.problems = h->problems.upload_range(b->problems + off, n * prob, off * prob, m * prob, st);
  d.states = d.problems ? h->states.upload_range(b->states + off, n * state, off * state, m * state, st) : nullptr;
  d.warm_start = d.states ? h->warm.upload_range(b->warm_start + off * nv, n * row, off * row, m * row, st) : nullptr;
  return d.warm_start ? NEO_MPC_OK : NEO_MPC_ERR_DEVICE;
}

// ... and with room for every output the batch asks for -> `d`: those m records as a device-pointer batch, without a
// footprint raster
int stage_up(neo_mpc_handle* h, const neo_mpc_batch* b, size_t off, size_t m, hipStream_t st, neo_mpc_batch& d,
             bool solution_is_input) {
  const size_t n = b->count, nv = 3 * (size_t)h->params.control_steps;
  d = *b;
  d.count = m;
  d.footprints = nullptr; d.footprint_points = 0;
  int rc = stage_records(h, b, off, m, st, d);
  if (rc) return rc;
  if ((rc = h->commands.reserve(n * sizeof(neo_mpc_command)))) return rc;
  d.commands = h->commands.as<neo_mpc_command>() + off;
  if (b->solution) {
    if (solution_is_input) {
      d.solution = h->solution.upload_range(b->solution + off * nv, n * nv * 8, off * nv * 8, m * nv * 8, st);
      if (!d.solution) return NEO_MPC_ERR_DEVICE;
    } else {
      if ((rc = h->solution.reserve(n * nv * 8))) return rc;
      d.solution = h->solution.as<double>() + off * nv;
    }
  }
  if (b->predicted_path) {
    if ((rc = h->path.reserve(n * nv * 8))) return rc;
    d.predicted_path = h->path.as<double>() + off * nv;
  }
  if (b->velocities) {
    if ((rc = h->vel.reserve(n * 24))) return rc;
    d.velocities = h->vel.as<double>() + off * 3;
  }
  return NEO_MPC_OK;
}

// The results of that range, queued on `st` behind the kernel and not waited for: with page-locked host arrays (hipHostMalloc /
// hipHostRegister / torch pin_memory) they are DMA transfers that overlap the host side of what follows; with pageable arrays
// the runtime stages them and each call returns when its copy is done
int stage_down(neo_mpc_handle* h, const neo_mpc_batch* b, size_t off, size_t m, hipStream_t st, bool solution_is_output) {
  const size_t nv = 3 * (size_t)h->params.control_steps;
  const size_t cmd = sizeof(neo_mpc_command), state = sizeof(neo_mpc_state), row = nv * 8;
  int rc;
  if ((rc = h->commands.download_range(b->commands + off, off * cmd, m * cmd, st))) return rc;
  if ((rc = h->states.download_range(b->states + off, off * state, m * state, st))) return rc;
  if ((rc = h->warm.download_range(b->warm_start + off * nv, off * row, m * row, st))) return rc;
  if (b->solution && solution_is_output &&
      (rc = h->solution.download_range(b->solution + off * nv, off * row, m * row, st)))
    return rc;
  if (b->predicted_path && (rc = h->path.download_range(b->predicted_path + off * nv, off * row, m * row, st)))
    return rc;
  if (b->velocities && (rc = h->vel.download_range(b->velocities + off * 3, off * 24, m * 24, st))) return rc;
  return NEO_MPC_OK;
}

// A whole host batch on the null stream, with its footprint raster
int stage_in(neo_mpc_handle* h, const neo_mpc_batch* b, neo_mpc_batch& d, bool solution_is_input) {
  int rc = stage_up(h, b, 0, b->count, nullptr, d, solution_is_input);
  if (rc) return rc;
  if (b->footprints && b->footprint_points) {
    if ((rc = check_vertices_finite(b->footprints, b->count, b->footprint_points, "footprint vertex", "instance"))) return rc;
    d.footprints = h->footprints.upload(b->footprints, b->count * b->footprint_points * 16, nullptr);
    if (!d.footprints) return NEO_MPC_ERR_DEVICE;
    d.footprint_points = b->footprint_points;
  }
  return NEO_MPC_OK;
}

// ... and back, waited for once
int stage_out(neo_mpc_handle* h, const neo_mpc_batch* b, bool solution_is_output) {
  int rc = stage_down(h, b, 0, b->count, nullptr, solution_is_output);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  return NEO_MPC_OK;
}

}  // namespace

extern "C" {

int neo_mpc_abi_version(void) { return NEO_MPC_ABI_VERSION; }
int neo_mpc_behaviour_version(void) { return NEO_MPC_BEHAVIOUR_VERSION; }

const char* neo_mpc_last_error(void) { return g_error.c_str(); }
int neo_mpc_last_error_code(void) { return g_error_code; }

int neo_mpc_default_params(neo_mpc_params* p) {
  if (!p) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null params");
  std::memset(p, 0, sizeof(*p));
  p->acc_x_limit = p->acc_y_limit = p->acc_theta_limit = 0.5;             // py:49-51
  p->min_vel_x = p->min_vel_y = p->min_vel_theta = -0.5;                   // py:53-56
  p->min_vel_trans = 0.5;                                                  // py:55 (sic)
  p->max_vel_x = p->max_vel_y = p->max_vel_trans = p->max_vel_theta = 0.5; // py:58-61
  p->w_trans = p->w_orient = p->w_control = p->w_terminal = p->w_costmap = 0.5;  // py:63-67
  p->w_footprint = 2000;                                                   // py:68
  p->waiting_time = 3.0;                                                   // py:70
  p->low_pass_gain = 0.5;                                                  // py:71
  p->opt_tolerance = 1e-5;                                                 // py:72
  p->prediction_horizon = 0.5;                                             // py:73
  p->control_steps = 3;                                                    // py:75
  p->max_iterations = 100;
  p->lbfgs_memory = 4;
  p->compat_flags = NEO_MPC_COMPAT_ODOM_YAW_GOAL_W;
  p->step_tolerance = 0.0;
  p->cost_tolerance = 0.0;
  p->kink_radius = 0.0;
  p->stall_step = 0.0;
  p->window_tolerance = 0.0;
  p->method = NEO_MPC_METHOD_AUTO;
  return NEO_MPC_OK;
}

neo_mpc_handle* neo_mpc_create(const neo_mpc_params* params, int device) {
  if (!params) { fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null params"); return nullptr; }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    fail(NEO_MPC_ERR_NO_DEVICE, "no HIP device visible (%s); this library has no CPU fallback",
         e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= count) { fail(NEO_MPC_ERR_INVALID_ARGUMENT, "device %d of %d", device, count); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { fail(NEO_MPC_ERR_DEVICE, "hipSetDevice(%d) failed", device); return nullptr; }
  neo_mpc_handle* h = new (std::nothrow) neo_mpc_handle();
  if (!h) { fail(NEO_MPC_ERR_DEVICE, "out of host memory"); return nullptr; }
  h->device = device;
  {  // the A/B switches of the measurement tools: the only place the library looks at the environment
    const char* e = getenv("NEO_MPC_SOLVE_WAVES");
    h->tuning.solve_waves = (e && atoi(e) >= 2 && atoi(e) <= 4) ? atoi(e) : 0;
    h->tuning.no_tame = getenv("NEO_MPC_NO_TAME_SPECIALISATION") != nullptr;
    h->tuning.dynamic_lds = getenv("NEO_MPC_DYNAMIC_LDS") != nullptr;
    h->no_chunks = getenv("NEO_MPC_NO_CHUNKS") != nullptr;
    e = getenv("NEO_MPC_HOST_PATH");
    h->auto_host_path = !e ? NEO_MPC_HOST_PATH_ZEROCOPY : !strcmp(e, "staged") ? NEO_MPC_HOST_PATH_STAGED
                        : !strcmp(e, "zerocopy_out") ? NEO_MPC_HOST_PATH_ZEROCOPY_OUT : NEO_MPC_HOST_PATH_ZEROCOPY;
  }
  if (apply_params(h, params, false) != NEO_MPC_OK) { neo_mpc_destroy(h); return nullptr; }
  return h;
}

void neo_mpc_destroy(neo_mpc_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (auto& f : h->in_flight) {
    if (f.busy) (void)hipEventSynchronize(f.done);
    if (f.done) (void)hipEventDestroy(f.done);
    if (f.stream) (void)hipStreamDestroy(f.stream);
  }
  for (hipStream_t cs : h->chunk_streams) if (cs) (void)hipStreamDestroy(cs);
  h->fence.destroy();
  h->world.destroy();
  if (h->pin) (void)hipHostFree(h->pin);
  delete h;   // (every DeviceBuffer frees its own memory, on the device set above)
}

int neo_mpc_set_params(neo_mpc_handle* h, const neo_mpc_params* params) {
  if (!h || !params) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return apply_params(h, params, true);
}

int neo_mpc_effective_method(const neo_mpc_handle* h) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  const int d = neo_rules_direction(&h->params);
  return d == NEO_DIRECTION_LBFGS ? NEO_MPC_METHOD_LBFGS : d == NEO_DIRECTION_DENSE ? NEO_MPC_METHOD_NEWTON : NEO_MPC_METHOD_RICCATI;
}

int neo_mpc_get_params(const neo_mpc_handle* h, neo_mpc_params* params) {
  if (!h || !params) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  *params = h->params;
  return NEO_MPC_OK;
}

int neo_mpc_set_costmap(neo_mpc_handle* h, const uint8_t* cells, uint32_t sx, uint32_t sy, double res, double ox,
                        double oy) {
  if (!h || !cells) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  const uint8_t* d_cells = h->raw_buf.upload(cells, (size_t)sx * sy);
  if (!d_cells) return NEO_MPC_ERR_DEVICE;
  // no synchronisation: `cells` has been consumed by the (blocking) copy above; K3 runs on the null
  // stream and every later launch waits for the fence (ingest's end_write) on its own stream
  return ingest(h, d_cells, 1, sx, sy, res, ox, oy, nullptr, nullptr);
}

int neo_mpc_set_costmap_device(neo_mpc_handle* h, const uint8_t* d_cells, uint32_t sx, uint32_t sy, double res,
                               double ox, double oy, void* stream) {
  if (!h || !d_cells) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return ingest(h, d_cells, 1, sx, sy, res, ox, oy, nullptr, stream);
}

int neo_mpc_set_costmap_pool_device(neo_mpc_handle* h, const uint8_t* d_cells, uint32_t count, uint32_t sx,
                                    uint32_t sy, double res, const double* d_origins, void* stream) {
  if (!h || !d_cells || !d_origins) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_pool_count(count)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return ingest(h, d_cells, count, sx, sy, res, 0.0, 0.0, d_origins, stream);
}

int neo_mpc_set_costmap_pool(neo_mpc_handle* h, const uint8_t* cells, uint32_t count, uint32_t sx, uint32_t sy,
                             double res, const double* origins) {
  if (!h || !cells || !origins) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  int rc = check_pool_count(count);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if ((rc = h->fence.wait_idle())) return rc;   // (batches in flight pair the old origins with the old cells to their end)
  const uint8_t* d_cells = h->raw_buf.upload(cells, (size_t)sx * sy * count);
  const double* d_origins = d_cells ? h->origins_buf.upload(origins, (size_t)count * 16) : nullptr;
  if (!d_origins) return NEO_MPC_ERR_DEVICE;
  return ingest(h, d_cells, count, sx, sy, res, 0.0, 0.0, d_origins, nullptr);
}

int neo_mpc_solve_batch_device_timed(neo_mpc_handle* h, const neo_mpc_batch* batch, void* stream, void* start_event,
                                     void* stop_event) {
  SolveArgs a;
  int rc = fill_args(h, batch, a);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));  // the stream and the buffers must belong to the handle's device
  if (h->order_count != 0 && h->order_count == batch->count) a.order = h->order_buf.as<const uint32_t>();
  return h->fence.read(stream, [&] { launch_solve(a, h->tuning, stream, start_event, stop_event); });
}

// Balanced dispatch for a fleet's next tick (K5): see k_dispatch_order.  Results do not depend on it.
int neo_mpc_balance_dispatch_device(neo_mpc_handle* h, const neo_mpc_command* d_previous_commands, size_t count, void* stream) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (!d_previous_commands || count == 0) { h->order_count = 0; return NEO_MPC_OK; }
  if (int rc = check_count(count, 0xffffffffull)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  // (the average is kept while calls of the same count follow one another; disarming or another count starts it afresh)
  const bool fresh = h->order_count != count;
  // disarmed until the new order is on its way: a reserve() that re-allocates for a larger count and then fails, or a launch
  // that fails, must not leave an order armed that points at a buffer nobody has written
  h->order_count = 0;
  int rc = h->order_buf.reserve(count * sizeof(uint32_t));
  if (rc) return rc;
  if ((rc = h->load_buf.reserve(count * sizeof(float)))) return rc;
  launch_dispatch_order(d_previous_commands, h->load_buf.as<float>(), h->order_buf.as<uint32_t>(), (uint32_t)count, fresh, stream);
  HIP_TRY(hipGetLastError());
  h->order_count = count;
  return NEO_MPC_OK;
}

// Test hook: the order and the averages K5 left in the handle.  K5 runs on the caller's stream, not through the fence:
// there is no writer to wait on, so the whole device is waited for.
int neo_mpc_get_dispatch_order(neo_mpc_handle* h, uint32_t* order_out, float* load_out, size_t* count_out) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  const size_t count = h->order_count;
  if (count_out) *count_out = count;
  if (count == 0 || (!order_out && !load_out)) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  if (order_out) HIP_TRY(hipMemcpy(order_out, h->order_buf.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
  // (a count that gets launch order -- k_dispatch_order's first branch -- never has its averages written: that memory is
  // nobody's to read)
  if (load_out && count % kDispatchSimds == 0 && count <= 4 * kDispatchSimds)
    HIP_TRY(hipMemcpy(load_out, h->load_buf.ptr, count * sizeof(float), hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

int neo_mpc_solve_batch_device(neo_mpc_handle* h, const neo_mpc_batch* batch, void* stream) {
  return neo_mpc_solve_batch_device_timed(h, batch, stream, nullptr, nullptr);
}

// neo_mpc_solve_batch for count <= kLatencyPathMaxCount without a footprint raster:
// [problems | states | warm | commands | velocities | solution | path] laid out once in a pinned block and
// mirrored in a device arena -- the whole input goes up in one copy, the whole output comes back in
// one, and the only synchronisation is the one that makes the results visible.
static int solve_batch_latency_path(neo_mpc_handle* h, const neo_mpc_batch* b) {
  const size_t n = b->count, nv = 3 * (size_t)h->params.control_steps;
  if (!h->pin) HIP_TRY(hipHostMalloc(&h->pin, kLatencyPathBytes, hipHostMallocDefault));
  int rc = h->arena.reserve(kLatencyPathBytes);
  if (rc) return rc;
  const size_t o_prob = 0, o_state = o_prob + n * sizeof(neo_mpc_problem), o_warm = o_state + n * sizeof(neo_mpc_state),
               o_cmd = o_warm + n * nv * 8, o_vel = o_cmd + n * sizeof(neo_mpc_command), o_sol = o_vel + n * 24,
               o_path = o_sol + (b->solution ? n * nv * 8 : 0), o_end = o_path + (b->predicted_path ? n * nv * 8 : 0);
  char* pin = (char*)h->pin;
  char* dev = h->arena.as<char>();
  memcpy(pin + o_prob, b->problems, n * sizeof(neo_mpc_problem));
  memcpy(pin + o_state, b->states, n * sizeof(neo_mpc_state));
  memcpy(pin + o_warm, b->warm_start, n * nv * 8);
  HIP_TRY(hipMemcpyAsync(dev, pin, o_cmd, hipMemcpyHostToDevice, nullptr));
  neo_mpc_batch d = *b;
  d.problems = (const neo_mpc_problem*)(dev + o_prob);
  d.states = (neo_mpc_state*)(dev + o_state);
  d.warm_start = (double*)(dev + o_warm);
  d.commands = (neo_mpc_command*)(dev + o_cmd);
  d.velocities = (double*)(dev + o_vel);
  if (b->solution) d.solution = (double*)(dev + o_sol);
  if (b->predicted_path) d.predicted_path = (double*)(dev + o_path);
  SolveArgs a;
  if ((rc = fill_args(h, &d, a))) return rc;
  if ((rc = solve_on(h, a, nullptr))) return rc;
  HIP_TRY(hipMemcpyAsync(pin + o_state, dev + o_state, o_end - o_state, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  memcpy(b->states, pin + o_state, n * sizeof(neo_mpc_state));
  memcpy(b->warm_start, pin + o_warm, n * nv * 8);
  memcpy(b->commands, pin + o_cmd, n * sizeof(neo_mpc_command));
  if (b->velocities) memcpy(b->velocities, pin + o_vel, n * 24);
  if (b->solution) memcpy(b->solution, pin + o_sol, n * nv * 8);
  if (b->predicted_path) memcpy(b->predicted_path, pin + o_path, n * nv * 8);
  return NEO_MPC_OK;
}

// Is `p` page-locked host memory the device can address (hipHostMalloc / hipHostRegister / neo_mpc_pin_host_memory /
// torch pin_memory)?  -> its device-side address.
static bool pinned_host(const void* p, size_t bytes, void** dev) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (unregistered memory: an error before ROCm 6)
  if (at.type != hipMemoryTypeHost || !at.devicePointer) return false;
  *dev = at.devicePointer;
  if (bytes > 1) {
    // ... to its LAST byte (a registered prefix of an arena, or count * stride beyond the pinned range, would fault on the
    // GPU instead of falling back to staging), and as ONE mapping: the device-side addresses are as far apart as the host's
    hipPointerAttribute_t last;
    const char* end = static_cast<const char*>(p) + bytes - 1;
    if (hipPointerGetAttributes(&last, end) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (last.type != hipMemoryTypeHost || !last.devicePointer) return false;
    if (static_cast<const char*>(last.devicePointer) - static_cast<const char*>(at.devicePointer) != (ptrdiff_t)(bytes - 1)) return false;
  }
  return true;
}

// neo_mpc_solve_batch when every array of the batch is page-locked: no staging copy at all.
//  kZeroCopy  K1 reads the request / state / warm-start records straight from the caller's arrays over PCIe -- they
//             are read once, at the start of each wave, as coalesced 8-byte-per-lane loads -- and writes commands,
//             state, warm start (and solution / path / velocities) straight back; the link is busy while other
//             waves compute.  One launch, one wait.
//  kZeroCopyOut  the inputs go up as three DMA copies into device staging, the results are written straight into the
//             caller's arrays by K1 (no D2H copies).
// NEO_MPC_HOST_PATH=staged|zerocopy|zerocopy_out in the environment of neo_mpc_create overrides what AUTO means (A/B runs).
enum HostPath { kStaged = NEO_MPC_HOST_PATH_STAGED, kZeroCopy = NEO_MPC_HOST_PATH_ZEROCOPY,
                kZeroCopyOut = NEO_MPC_HOST_PATH_ZEROCOPY_OUT };
static HostPath host_path_mode(const neo_mpc_handle* h) {
  return (HostPath)(h->host_path != NEO_MPC_HOST_PATH_AUTO ? h->host_path : h->auto_host_path);
}

static int solve_batch_zero_copy(neo_mpc_handle* h, const neo_mpc_batch* b, const neo_mpc_batch& dev, HostPath mode) {
  neo_mpc_batch d = dev;          // every pointer: the device-side address of the caller's page-locked array
  SolveArgs a;
  int rc;
  auto bail = [](int code) { (void)hipStreamSynchronize(nullptr); return code; };
  if (mode == kZeroCopyOut && (rc = stage_records(h, b, 0, b->count, nullptr, d))) return bail(rc);
  if ((rc = fill_args(h, &d, a))) return bail(rc);
  a.states_out = dev.states; a.warm_out = dev.warm_start;
  if ((rc = solve_on(h, a, nullptr))) return bail(rc);
  HIP_TRY(hipStreamSynchronize(nullptr));   // kernel end = system-scope release: the results are in the caller's arrays
  return NEO_MPC_OK;
}

// Is every array of the host batch page-locked over its whole extent?  -> `dv`: the batch with the device-side addresses.
static bool batch_page_locked(const neo_mpc_handle* h, const neo_mpc_batch* batch, neo_mpc_batch& dv) {
  dv = *batch;
  const size_t n = batch->count, nv = 3 * (size_t)h->params.control_steps;
  bool all = pinned_host(batch->problems, n * sizeof(neo_mpc_problem), (void**)&dv.problems) &&
             pinned_host(batch->states, n * sizeof(neo_mpc_state), (void**)&dv.states) &&
             pinned_host(batch->warm_start, n * nv * 8, (void**)&dv.warm_start) &&
             pinned_host(batch->commands, n * sizeof(neo_mpc_command), (void**)&dv.commands);
  if (all && batch->solution) all = pinned_host(batch->solution, n * nv * 8, (void**)&dv.solution);
  if (all && batch->predicted_path) all = pinned_host(batch->predicted_path, n * nv * 8, (void**)&dv.predicted_path);
  if (all && batch->velocities) all = pinned_host(batch->velocities, n * 24, (void**)&dv.velocities);
  if (all && batch->footprints && batch->footprint_points)
    all = pinned_host(batch->footprints, n * batch->footprint_points * 16, (void**)&dv.footprints);
  return all;
}

// A staged host batch of kChunkedMinCount instances or more goes through in kChunks pieces on two streams: piece c + 1
// is copied up and launched before piece c's results are copied back, so copies and kernels of neighbouring pieces
// overlap (with pageable arrays the runtime's bounce copies block the host, the kernels run behind them; with
// page-locked arrays everything is asynchronous).  The instances are independent: the pieces' results are the batch's.
static int solve_batch_staged_chunks(neo_mpc_handle* h, const neo_mpc_batch* b) {
  const size_t n = b->count;
  for (hipStream_t& cs : h->chunk_streams)
    if (!cs) HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  auto bail = [&](int code) {
    for (hipStream_t cs : h->chunk_streams) (void)hipStreamSynchronize(cs);
    return code;
  };
  const size_t per = ((n + kChunks - 1) / kChunks + 63) & ~(size_t)63;
  auto piece = [&](size_t c, size_t& off, size_t& m) { off = c * per; m = off < n ? (n - off < per ? n - off : per) : 0; };
  auto up_and_launch = [&](size_t c) -> int {
    size_t off, m;
    piece(c, off, m);
    if (!m) return NEO_MPC_OK;
    hipStream_t st = h->chunk_streams[c & 1];
    neo_mpc_batch d;
    SolveArgs a;
    int r = stage_up(h, b, off, m, st, d, false);   // (the first piece sizes the staging buffers for the whole batch)
    if (r || (r = fill_args(h, &d, a))) return r;
    return solve_on(h, a, st);
  };
  auto down = [&](size_t c) -> int {
    size_t off, m;
    piece(c, off, m);
    return m ? stage_down(h, b, off, m, h->chunk_streams[c & 1], true) : NEO_MPC_OK;
  };
  int rc;
  if ((rc = up_and_launch(0))) return bail(rc);
  for (size_t c = 0; c < kChunks; ++c) {
    if (c + 1 < kChunks && (rc = up_and_launch(c + 1))) return bail(rc);
    if ((rc = down(c))) return bail(rc);
  }
  for (hipStream_t cs : h->chunk_streams) HIP_TRY(hipStreamSynchronize(cs));
  return NEO_MPC_OK;
}

// neo_mpc_problem.skip was reserved[0] in ABI 1, whose header never asked for zeroed reserved bytes: a host batch whose
// skip fields hold anything but 0 or 1 is refused instead of having robots silently left out (one int per record; device
// batches cannot be scanned -- K1 and K2 act on skip == 1 alone there).
static int check_skip_fields(const neo_mpc_batch* batch) {
  for (size_t i = 0; i < batch->count; ++i)
    if ((uint32_t)batch->problems[i].skip > 1u)
      return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "problems[%zu].skip = %d: must be 0 or 1 (reserved fields must be zeroed)", i,
                  batch->problems[i].skip);
  return NEO_MPC_OK;
}

int neo_mpc_solve_batch(neo_mpc_handle* h, const neo_mpc_batch* batch) {
  SolveArgs a;
  int rc = fill_args(h, batch, a);  // validates
  if (rc) return rc;
  if (batch->count == 0) return NEO_MPC_OK;
  if ((rc = check_skip_fields(batch))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if (batch->count <= kLatencyPathMaxCount && !batch->footprints)
    return solve_batch_latency_path(h, batch);
  if (host_path_mode(h) != kStaged) {
    // page-locked arrays throughout (a fleet server's request arena): K1 works on them in place
    neo_mpc_batch dv;
    if (batch_page_locked(h, batch, dv)) return solve_batch_zero_copy(h, batch, dv, host_path_mode(h));
  }
  if (batch->count >= kChunkedMinCount && !(batch->footprints && batch->footprint_points) && !h->no_chunks)
    return solve_batch_staged_chunks(h, batch);
  neo_mpc_batch d;
  // (the staging copies are asynchronous: no way out of here while one may still be reading the caller's buffers)
  auto bail = [](int code) { (void)hipStreamSynchronize(nullptr); return code; };
  if ((rc = stage_in(h, batch, d, false))) return bail(rc);
  if ((rc = fill_args(h, &d, a))) return bail(rc);
  if ((rc = solve_on(h, a, nullptr))) return bail(rc);
  return bail(stage_out(h, batch, true));   // (queued behind the kernel on the null stream, one wait at the end)
}

// The two halves of the reference's `async_send_request(request)` ... `result.get()` (cpp:248-250) for a batch: begin
// enqueues K1 on a stream of its own -- the batch's arrays are page-locked and worked on in place, as in
// neo_mpc_solve_batch -- and returns; wait blocks until that batch's results are in the caller's arrays.  With two
// batches in flight the launch latency, the wait for the records over PCIe and the host's own work between calls
// hide under the other batch's kernel.
int neo_mpc_solve_batch_begin(neo_mpc_handle* h, const neo_mpc_batch* batch, uint32_t* ticket) {
  if (!ticket) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null ticket");
  *ticket = 0;
  SolveArgs a;
  int rc = fill_args(h, batch, a);  // validates
  if (rc) return rc;
  if (batch->count == 0) return NEO_MPC_OK;   // (ticket 0: nothing to wait for)
  if ((rc = check_skip_fields(batch))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  neo_mpc_batch dv;
  if (!batch_page_locked(h, batch, dv))
    return fail(NEO_MPC_ERR_UNSUPPORTED, "neo_mpc_solve_batch_begin works on page-locked arrays in place: pin the batch's "
                "arrays (neo_mpc_pin_host_memory) or call neo_mpc_solve_batch");
  neo_mpc_handle::InFlight* slot = nullptr;
  uint32_t index = 0;
  for (uint32_t k = 0; k < NEO_MPC_MAX_BATCHES_IN_FLIGHT; ++k)
    if (!h->in_flight[k].busy) { slot = &h->in_flight[k]; index = k; break; }
  if (!slot) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "%d batches in flight already: wait for one", NEO_MPC_MAX_BATCHES_IN_FLIGHT);
  if (!slot->stream) HIP_TRY(hipStreamCreateWithFlags(&slot->stream, hipStreamNonBlocking));
  // (system-scope release: the results are visible to the host after hipEventSynchronize also in non-coherent pinned
  // memory -- hipHostMallocNonCoherent, HIP_HOST_COHERENT=0)
  if (!slot->done) HIP_TRY(hipEventCreateWithFlags(&slot->done, hipEventDisableTiming | hipEventReleaseToSystem));
  if ((rc = fill_args(h, &dv, a))) return rc;
  a.states_out = dv.states; a.warm_out = dv.warm_start;
  // from here on a kernel may be writing the caller's arrays: no way out without a ticket unless it has been waited for
  auto bail = [&](int code) { (void)hipStreamSynchronize(slot->stream); return code; };
  if ((rc = solve_on(h, a, slot->stream))) return bail(rc);
  if (hipEventRecord(slot->done, slot->stream) != hipSuccess) return bail(fail(NEO_MPC_ERR_DEVICE, "hipEventRecord failed"));
  slot->busy = true;
  *ticket = index + 1;
  return NEO_MPC_OK;
}

int neo_mpc_solve_batch_wait(neo_mpc_handle* h, uint32_t ticket) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (ticket == 0) return NEO_MPC_OK;
  if (ticket > NEO_MPC_MAX_BATCHES_IN_FLIGHT || !h->in_flight[ticket - 1].busy)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "ticket %u names no batch in flight", ticket);
  neo_mpc_handle::InFlight& f = h->in_flight[ticket - 1];
  f.busy = false;
  HIP_TRY(hipEventSynchronize(f.done));   // kernel end = system-scope release: the results are in the caller's arrays
  return NEO_MPC_OK;
}

int neo_mpc_set_host_path(neo_mpc_handle* h, int mode) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (mode < NEO_MPC_HOST_PATH_AUTO || mode > NEO_MPC_HOST_PATH_ZEROCOPY_OUT)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown host path %d", mode);
  h->host_path = mode;
  return NEO_MPC_OK;
}

// Page-lock / release a host array of the caller's (hipHostRegister / hipHostUnregister behind a C signature, for
// callers built without the HIP headers -- the nav2 plugin is plain g++).
int neo_mpc_pin_host_memory(void* ptr, size_t bytes) {
  if (!ptr || bytes == 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
  return NEO_MPC_OK;
}
int neo_mpc_unpin_host_memory(void* ptr) {
  if (!ptr) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipHostUnregister(ptr));
  return NEO_MPC_OK;
}

int neo_mpc_postprocess_batch(neo_mpc_handle* h, const neo_mpc_batch* batch, const int32_t* success) {
  SolveArgs a;
  int rc = fill_args(h, batch, a);
  if (rc) return rc;
  if (!batch->solution) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "postprocess needs batch->solution (x.x)");
  if (batch->count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  neo_mpc_batch d;
  auto bail = [](int code) { (void)hipStreamSynchronize(nullptr); return code; };
  if ((rc = stage_in(h, batch, d, true))) return bail(rc);
  if ((rc = fill_args(h, &d, a))) return bail(rc);
  if (success && !(a.success = h->success.upload(success, batch->count * 4))) return bail(NEO_MPC_ERR_DEVICE);
  if ((rc = h->fence.read(nullptr, [&] { launch_postprocess(a, nullptr); }))) return bail(rc);
  return bail(stage_out(h, batch, false));
}

int neo_mpc_objective_batch(neo_mpc_handle* h, const neo_mpc_problem* problems, const double* u, double* cost_out,
                            size_t count) {
  if (!h || !problems || !u || !cost_out) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->has_map) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_costmap has not been called");
  if (count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nv = 3 * (size_t)h->params.control_steps;
  int rc;
  ObjectiveArgs a;
  std::memset(&a, 0, sizeof(a));
  if ((rc = h->cost.reserve(count * 8))) return rc;
  if (!(a.problems = h->problems.upload(problems, count * sizeof(neo_mpc_problem)))) return NEO_MPC_ERR_DEVICE;
  if (!(a.u = h->u.upload(u, count * nv * 8))) return NEO_MPC_ERR_DEVICE;
  a.cost = h->cost.as<double>();
  a.term_table = h->term_buf.as<const double>();
  a.count = (uint32_t)count;
  a.p = h->dp; a.map = h->map;
  a.w_trans = h->params.w_trans; a.w_orient = h->params.w_orient; a.w_control = h->params.w_control;
  a.w_terminal = h->params.w_terminal; a.w_costmap = h->params.w_costmap;
  if ((rc = h->fence.read(nullptr, [&] { launch_objective(a, nullptr); }))) return rc;
  HIP_TRY(hipMemcpy(cost_out, h->cost.ptr, count * 8, hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

// The gradient / direction hooks: K1 itself with `u` as the warm start of instances whose goal is unchanged (no reset), stopped
// right after its first gradient pass (DevParams.max_it = kDumpGradient), or after the direction of `iteration`: the vector
// comes out of `solution`
static int hook_batch(neo_mpc_handle* h, const neo_mpc_problem* problems, const double* u, double* out, size_t count,
                      int max_it) {
  if (!h || !problems || !u || !out) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->has_map) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_costmap has not been called");
  if (count == 0) return NEO_MPC_OK;
  int rc = check_count(count);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nv = 3 * (size_t)h->params.control_steps;
  std::vector<neo_mpc_state> st(count);
  std::memset(st.data(), 0, count * sizeof(neo_mpc_state));
  for (size_t i = 0; i < count; ++i) {
    for (int k = 0; k < 3; ++k) st[i].old_goal[k] = problems[i].goal_xyz[k];
    for (int k = 0; k < 4; ++k) st[i].old_goal[3 + k] = problems[i].goal_q[k];
    st[i].has_old_goal = 1;
  }
  neo_mpc_batch b, d;   // the hook's inputs as a host batch whose only output is the solution
  std::memset(&b, 0, sizeof(b));
  b.count = count;
  b.problems = problems; b.states = st.data(); b.warm_start = const_cast<double*>(u); b.solution = out;
  SolveArgs a;
  // (the staging copies are asynchronous and `st` is this call's own)
  auto bail = [](int code) { (void)hipStreamSynchronize(nullptr); return code; };
  if ((rc = stage_up(h, &b, 0, count, nullptr, d, false))) return bail(rc);
  if ((rc = fill_args(h, &d, a))) return bail(rc);
  a.p.max_it = max_it;
  // NaN rows for instances that stop before the dump
  if ((rc = hip_check(hipMemsetAsync(d.solution, 0xFF, count * nv * 8, nullptr), "hipMemsetAsync"))) return bail(rc);
  if ((rc = solve_on(h, a, nullptr))) return bail(rc);
  // (a blocking copy on the null stream, behind the staging copies and the kernel)
  return bail(hip_check(hipMemcpy(out, d.solution, count * nv * 8, hipMemcpyDeviceToHost), "hipMemcpy"));
}

int neo_mpc_gradient_batch(neo_mpc_handle* h, const neo_mpc_problem* problems, const double* u, double* grad_out,
                           size_t count) {
  return hook_batch(h, problems, u, grad_out, count, kDumpGradient);
}
int neo_mpc_direction_batch(neo_mpc_handle* h, const neo_mpc_problem* problems, const double* u, double* dir_out,
                            size_t count, int iteration) {
  if (iteration < 0 || iteration > 1000) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "iteration %d", iteration);
  return hook_batch(h, problems, u, dir_out, count, kDumpGradient + 1 + iteration);
}

// K4.
static int check_plan_batch(const neo_mpc_handle* h, const neo_mpc_lookahead_params* lp, const neo_mpc_plan_batch* b) {
  if (!h || !lp || !b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (b->count > 0 && (!b->plan_poses || !b->plan_offsets || !b->robot_poses || !b->slow_down || !b->carrots))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "plan_poses/plan_offsets/robot_poses/slow_down/carrots must not be null");
  return check_count(b->count);
}

int neo_mpc_select_carrots_device(neo_mpc_handle* h, const neo_mpc_lookahead_params* lp,
                                  const neo_mpc_plan_batch* b, void* stream) {
  int rc = check_plan_batch(h, lp, b);
  if (rc) return rc;
  CarrotArgs a;
  a.lp = *lp;
  a.b = *b;
  HIP_TRY(hipSetDevice(h->device));
  launch_carrots(a, stream);
  HIP_TRY(hipGetLastError());
  return NEO_MPC_OK;
}

int neo_mpc_select_carrots(neo_mpc_handle* h, const neo_mpc_lookahead_params* lp, const neo_mpc_plan_batch* b) {
  int rc = check_plan_batch(h, lp, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = b->count;
  const size_t total = b->plan_offsets[n];
  if ((rc = h->plan_poses.reserve(total * 24 + 8))) return rc;   // (never empty: a fleet without a plan pose stages nothing)
  if ((rc = h->carrots.reserve(n * sizeof(neo_mpc_carrot)))) return rc;
  CarrotArgs a;
  a.lp = *lp;
  a.b = *b;
  a.b.carrots = h->carrots.as<neo_mpc_carrot>();
  if (!(a.b.plan_poses = h->plan_poses.upload(b->plan_poses, total * 24))) return NEO_MPC_ERR_DEVICE;
  if (!(a.b.plan_offsets = h->plan_offsets.upload(b->plan_offsets, (n + 1) * 4))) return NEO_MPC_ERR_DEVICE;
  if (!(a.b.robot_poses = h->poses.upload(b->robot_poses, n * 24))) return NEO_MPC_ERR_DEVICE;
  if (!(a.b.slow_down = h->slow_down.upload(b->slow_down, n * 4))) return NEO_MPC_ERR_DEVICE;
  if (b->footprint_costs && !(a.b.footprint_costs = h->fp_costs.upload(b->footprint_costs, n * 8))) return NEO_MPC_ERR_DEVICE;
  if (b->problems && !(a.b.problems = h->problems.upload(b->problems, n * sizeof(neo_mpc_problem)))) return NEO_MPC_ERR_DEVICE;
  launch_carrots(a, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(b->carrots, h->carrots.ptr, n * sizeof(neo_mpc_carrot), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b->slow_down, h->slow_down.ptr, n * 4, hipMemcpyDeviceToHost));
  if (b->problems)
    HIP_TRY(hipMemcpy(b->problems, h->problems.ptr, n * sizeof(neo_mpc_problem), hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

// K6.  What both gate entry points check: the record's shape, never a value behind a pointer.
static int check_footprint_batch(const neo_mpc_handle* h, const neo_mpc_footprint_batch* b) {
  if (!h || !b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->has_map) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_costmap has not been called");
  int rc = check_footprint_shape(b->footprint_points, b->per_robot_footprints);
  if (rc || (rc = check_count(b->count))) return rc;
  if (b->count > 0 && (!b->footprint || !b->footprint_costs))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "footprint/footprint_costs must not be null");
  if (b->count > 0 && !b->poses && !b->problems)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "poses and problems are both null: no pose to place the footprint at");
  return NEO_MPC_OK;
}

// `d`: the record with device pointers
static int gate(neo_mpc_handle* h, const neo_mpc_footprint_batch& d, void* stream) {
  FootprintGateArgs a;
  std::memset(&a, 0, sizeof(a));
  a.footprint = d.footprint; a.poses = d.poses; a.map_indices = d.map_indices; a.problems = d.problems;
  a.footprint_costs = d.footprint_costs; a.footprints_out = d.footprints_out;
  a.count = (uint32_t)d.count; a.footprint_points = d.footprint_points; a.per_robot = d.per_robot_footprints;
  a.map = h->map;
  return h->fence.read(stream, [&] { launch_footprint_gate(a, stream); });
}

int neo_mpc_footprint_gate_device(neo_mpc_handle* h, const neo_mpc_footprint_batch* b, void* stream) {
  int rc = check_footprint_batch(h, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  return gate(h, *b, stream);
}

int neo_mpc_footprint_gate(neo_mpc_handle* h, const neo_mpc_footprint_batch* b) {
  int rc = check_footprint_batch(h, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  const size_t n = b->count, np = b->footprint_points, polygons = b->per_robot_footprints ? n : 1;
  // the values the device variant takes as they come are looked at here
  if ((rc = check_vertices_finite(b->footprint, polygons, np, "footprint vertex", "polygon"))) return rc;
  const int pool = (b->map_indices || b->problems) ? h->map.pool_count : 0;
  auto check_map_index = [&](size_t i) {
    const int32_t idx = pool <= 0 ? 0 : b->map_indices ? b->map_indices[i] : b->problems[i].map_index;
    if (idx >= 0 && (pool <= 0 || idx < pool)) return (int)NEO_MPC_OK;
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "map index %d of robot %zu outside the pool of %d maps", idx, i, pool);
  };
  if ((rc = check_poses_finite(b->poses, b->problems, n, check_map_index))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if ((rc = h->fp_costs.reserve(n * 8))) return rc;
  neo_mpc_footprint_batch d = *b;
  d.footprint_costs = h->fp_costs.as<double>();
  if (!(d.footprint = h->verts.upload(b->footprint, polygons * np * 16))) return NEO_MPC_ERR_DEVICE;
  if (b->poses && !(d.poses = h->poses.upload(b->poses, n * 24))) return NEO_MPC_ERR_DEVICE;
  if (b->map_indices && !(d.map_indices = h->gate_indices.upload(b->map_indices, n * 4))) return NEO_MPC_ERR_DEVICE;
  if (b->problems && !(d.problems = h->problems.upload(b->problems, n * sizeof(neo_mpc_problem)))) return NEO_MPC_ERR_DEVICE;
  if (b->footprints_out) {
    if ((rc = h->gate_polygons_out.reserve(n * np * 16))) return rc;
    d.footprints_out = h->gate_polygons_out.as<double>();
  }
  if ((rc = gate(h, d, nullptr))) return rc;
  // (blocking copies on the null stream, behind the kernel; the records come back whole -- the kernel wrote footprint_cost alone)
  HIP_TRY(hipMemcpy(b->footprint_costs, h->fp_costs.ptr, n * 8, hipMemcpyDeviceToHost));
  if (b->footprints_out) HIP_TRY(hipMemcpy(b->footprints_out, h->gate_polygons_out.ptr, n * np * 16, hipMemcpyDeviceToHost));
  if (b->problems) HIP_TRY(hipMemcpy(b->problems, h->problems.ptr, n * sizeof(neo_mpc_problem), hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

// K7.  The world map: the handle's own device copy, from host cells (stream == nullptr, blocking) or device cells (on `stream`).
static int set_world_map(neo_mpc_handle* h, const uint8_t* cells, bool on_device, uint32_t sx, uint32_t sy, double res, double ox,
                         double oy, void* stream) {
  if (!h || !cells) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (sx == 0 || sy == 0 || sx > (1u << 20) || sy > (1u << 20) || !(res > 0.0) || !std::isfinite(res) || !std::isfinite(ox) ||
      !std::isfinite(oy))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "bad world map geometry %ux%u res %g origin (%g, %g)", sx, sy, res, ox, oy);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)sx * sy;
  WorldMap& w = h->world;
  int rc = w.begin_write(h->fence, on_device, st);
  if (rc) return rc;
  h->world_scan.live_valid = false;   // (K12: the next update composes the new map; until then the roll reads this one)
  rc = w.buf.reserve(bytes);
  if (rc) { w.has = false; return rc; }   // (a failed re-allocation has let the old copy go)
  if (on_device) HIP_TRY(hipMemcpyAsync(w.buf.ptr, cells, bytes, hipMemcpyDeviceToDevice, st));
  else HIP_TRY(hipMemcpy(w.buf.ptr, cells, bytes, hipMemcpyHostToDevice));
  if ((rc = w.end_write(st))) return rc;
  w.size_x = (int32_t)sx; w.size_y = (int32_t)sy;
  w.resolution = res; w.origin_x = ox; w.origin_y = oy;
  w.has = true;
  // (K12: a layer of another size is no layer of this world -- the next update resets it anyway, and until then
  // neo_mpc_get_world_scan_layer has nothing of the size its caller expects)
  if (h->world_scan.size_x != w.size_x || h->world_scan.size_y != w.size_y) h->world_scan.valid = false;
  return NEO_MPC_OK;
}

int neo_mpc_set_world_map(neo_mpc_handle* h, const uint8_t* cells, uint32_t sx, uint32_t sy, double res, double ox, double oy) {
  return set_world_map(h, cells, false, sx, sy, res, ox, oy, nullptr);
}

int neo_mpc_set_world_map_device(neo_mpc_handle* h, const uint8_t* d_cells, uint32_t sx, uint32_t sy, double res, double ox,
                                 double oy, void* stream) {
  return set_world_map(h, d_cells, true, sx, sy, res, ox, oy, stream);
}

// What both roll entry points check: the record's shape, never a value behind a pointer.
static int check_window_batch(const neo_mpc_handle* h, const neo_mpc_window_batch* w) {
  if (!h || !w) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->world.has) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_world_map has not been called");
  if (w->reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_window_batch.reserved must be zero (got %u)", w->reserved);
  if (w->outside_value > 255) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "outside_value %u is no cell value (0 .. 255)", w->outside_value);
  if (w->count > NEO_MPC_MAX_POOL_MAPS)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "%zu windows: a costmap pool holds at most %u maps", w->count, NEO_MPC_MAX_POOL_MAPS);
  if (w->size_x == 0 || w->size_y == 0 || w->size_x > (1u << 20) || w->size_y > (1u << 20))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "bad window size %ux%u", w->size_x, w->size_y);
  if (!(w->resolution > 0.0) || !std::isfinite(w->resolution))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "window resolution %g must be positive and finite", w->resolution);
  if (w->count > 0 && !w->origins) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "origins must not be null");
  return PaddedMap(w->size_x, w->size_y, kPoolBorder).check("window");
}

// `d`: the record with device pointers.  Orders itself like ingest() and leaves the handle's costmap as this pool.
static int roll(neo_mpc_handle* h, const neo_mpc_window_batch& d, void* stream) {
  const int sx = (int)d.size_x, sy = (int)d.size_y, count = (int)d.count;
  const PaddedMap g(d.size_x, d.size_y, kPoolBorder);
  const int tab_x = (sx + 15) & ~15, tab_stride = tab_x + ((sy + 3) & ~3);
  // the roll of every tick -- same geometry, count and origins as the previous one -- finds its buffers and the derived
  // constants in place: nothing is allocated (a re-allocation synchronises), so the call can be captured in a graph
  const bool same = h->has_map && h->rolled && h->map.pool_count == count && h->map.size_x == sx && h->map.size_y == sy &&
                    h->map.resolution == d.resolution && h->map.pool_origins == d.origins;
  int rc;
  if (!same) {
    if ((rc = h->map_buf.reserve(g.stride * count))) return rc;
    if ((rc = h->roll_tables.reserve((size_t)count * tab_stride * sizeof(int32_t)))) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  // behind the previous ingest or roll, every launch still reading the old map (it reads `origins` too: the device variant
  // rewrites them in-stream behind these waits) and the world map's copy
  if ((rc = h->fence.begin_write(st))) return rc;
  if ((rc = h->world.wait_writer(st))) return rc;
  RollArgs a;
  std::memset(&a, 0, sizeof(a));
  a.poses = d.poses; a.problems = d.poses ? nullptr : d.problems; a.origins = d.origins;
  a.tables = h->roll_tables.as<int32_t>();
  // (K12: while an update's composition is current the windows are cut from it -- same geometry, same event)
  a.world = h->world_scan.live_valid ? h->world_scan.live.as<const uint8_t>() : h->world.buf.as<const uint8_t>();
  a.dst = h->map_buf.as<uint8_t>();
  a.res = d.resolution; a.wres = h->world.resolution; a.wox = h->world.origin_x; a.woy = h->world.origin_y;
  a.dst_stride = (int64_t)g.stride;
  a.wsx = h->world.size_x; a.wsy = h->world.size_y;
  a.size_x = sx; a.size_y = sy; a.pitch = g.pitch; a.rows = g.rows; a.border = g.border;
  a.tab_x = tab_x; a.tab_stride = tab_stride;
  a.count = (uint32_t)count; a.outside = d.outside_value;
  launch_roll(a, stream);
  HIP_TRY(hipGetLastError());
  if ((rc = h->fence.end_write(st))) return rc;
  if (!same) adopt_map(h, g, (uint32_t)d.count, d.resolution, 0.0, 0.0, d.origins, true);
  return NEO_MPC_OK;
}

int neo_mpc_roll_costmap_pool_device(neo_mpc_handle* h, const neo_mpc_window_batch* w, void* stream) {
  int rc = check_window_batch(h, w);
  if (rc) return rc;
  if (w->count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  return roll(h, *w, stream);
}

int neo_mpc_roll_costmap_pool(neo_mpc_handle* h, const neo_mpc_window_batch* w) {
  int rc = check_window_batch(h, w);
  if (rc) return rc;
  if (w->count == 0) return NEO_MPC_OK;
  const size_t n = w->count;
  // the values the device variant takes as they come are looked at here
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(w->origins[2 * i]) || !std::isfinite(w->origins[2 * i + 1]))
      return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "the origin of window %zu is not finite", i);
  std::vector<double> poses;
  if (w->poses || w->problems) {
    poses.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const double x = w->poses ? w->poses[3 * i] : w->problems[i].cur_xy[0];
      const double y = w->poses ? w->poses[3 * i + 1] : w->problems[i].cur_xy[1];
      if (!std::isfinite(x) || !std::isfinite(y)) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "the pose of window %zu is not finite", i);
      poses[3 * i] = x; poses[3 * i + 1] = y; poses[3 * i + 2] = 0.0;
    }
  }
  HIP_TRY(hipSetDevice(h->device));
  // origins_buf is rewritten with a blocking copy on the null stream: every launch that may still read it -- a pool of
  // neo_mpc_set_costmap_pool's or of an earlier roll -- is waited for first
  if ((rc = h->fence.wait_idle())) return rc;
  neo_mpc_window_batch d = *w;
  d.poses = nullptr; d.problems = nullptr;
  if (!(d.origins = h->origins_buf.upload(w->origins, n * 16))) return NEO_MPC_ERR_DEVICE;
  if (!poses.empty() && !(d.poses = h->poses.upload(poses.data(), n * 24))) return NEO_MPC_ERR_DEVICE;
  if ((rc = roll(h, d, nullptr))) { (void)hipStreamSynchronize(nullptr); return rc; }
  // (a blocking copy on the null stream, behind the two kernels)
  HIP_TRY(hipMemcpy(w->origins, h->origins_buf.ptr, n * 16, hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

// Maps first .. first + count - 1 of those at `base` (rows `pitch` bytes apart, maps `stride`) -> cells_out (if asked for),
// sx * sy bytes each: a strided copy per map, border and pitch stay behind
static int download_maps(const uint8_t* base, size_t pitch, size_t stride, size_t sx, size_t sy, uint32_t first, uint32_t count,
                         uint8_t* cells_out) {
  for (uint32_t k = 0; cells_out && k < count; ++k)
    HIP_TRY(hipMemcpy2D(cells_out + (size_t)k * sx * sy, sx, base + (size_t)(first + k) * stride, pitch, sx, sy, hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

int neo_mpc_get_costmap_pool(neo_mpc_handle* h, uint32_t first, uint32_t count, uint8_t* cells_out, double* origins_out) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (!h->has_map) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_costmap has not been called");
  const uint32_t maps = h->map.pool_count > 0 ? (uint32_t)h->map.pool_count : 1u;
  if (first > maps || count > maps - first)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "maps [%u, %u + %u) outside the pool of %u", first, first, count, maps);
  if (count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  int rc = h->fence.wait_writer_host();   // the ingest, roll or stamp in flight
  if (rc) return rc;
  const DevMap& m = h->map;
  if ((rc = download_maps(m.cells, m.pitch, m.pool_stride, m.size_x, m.size_y, first, count, cells_out))) return rc;
  if (origins_out) {
    if (h->map.pool_count > 0)
      HIP_TRY(hipMemcpy(origins_out, h->map.pool_origins + 2 * (size_t)first, (size_t)count * 16, hipMemcpyDeviceToHost));
    else { origins_out[0] = h->map.origin_x; origins_out[1] = h->map.origin_y; }
  }
  return NEO_MPC_OK;
}

int neo_mpc_get_world_map(neo_mpc_handle* h, uint8_t* cells_out, uint32_t* size_x, uint32_t* size_y, double* resolution,
                          double* origin_x, double* origin_y) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (!h->world.has) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_world_map has not been called");
  WorldMap& w = h->world;
  if (size_x) *size_x = (uint32_t)w.size_x;
  if (size_y) *size_y = (uint32_t)w.size_y;
  if (resolution) *resolution = w.resolution;
  if (origin_x) *origin_x = w.origin_x;
  if (origin_y) *origin_y = w.origin_y;
  if (!cells_out) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (int rc = w.wait_writer_host()) return rc;   // the copy or inflation in flight
  HIP_TRY(hipMemcpy(cells_out, w.buf.ptr, (size_t)w.size_x * (size_t)w.size_y, hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

int neo_mpc_inflation_costs(double res, double ins, double infl, double csf, uint8_t* table_out, size_t capacity,
                            uint32_t* cells_out) {
  if (!(res > 0.0) || !std::isfinite(res))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "resolution %g must be positive and finite", res);
  int reach;
  if (int rc = inflation_reach(res, ins, infl, csf, "", &reach)) return rc;
  if (cells_out) *cells_out = (uint32_t)reach;
  if (table_out) {
    if (capacity < (size_t)reach * reach + 1)
      return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "the table needs %zu bytes, capacity is %zu", (size_t)reach * reach + 1, capacity);
    stamp_costs(res, ins, csf, reach, table_out);
  }
  return NEO_MPC_OK;
}

// The refusals K8 and K10 share, behind each one's own: the handle's pool, one robot per window, the reach
static int check_pool_batch(const neo_mpc_handle* h, size_t count, double ins, double infl, double csf) {
  if (!h->has_map) return fail(NEO_MPC_ERR_NO_COSTMAP, "the handle holds no costmap");
  if (h->map.pool_count <= 0) return fail(NEO_MPC_ERR_UNSUPPORTED, "the handle holds a single costmap, not a pool");
  if (count > 0 && count != (size_t)h->map.pool_count)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "%zu robots for a pool of %d windows: they are one to one", count, h->map.pool_count);
  return inflation_reach(h->map.resolution, ins, infl, csf, "", nullptr);
}

// The end of a synchronous variant of K8 to K12: the null stream is waited for whether or not the enqueue failed (`rc`) -> the first error
static int finish_on_null_stream(int rc) {
  if (rc) { (void)hipStreamSynchronize(nullptr); return rc; }
  HIP_TRY(hipStreamSynchronize(nullptr));
  return NEO_MPC_OK;
}

// ---------------------------------------------------------------------------------------------- a fleet's outlines
// K8, K12.  What neo_mpc_stamp_batch and neo_mpc_fleet_clear say of the robots' outlines, in one form: polygons in the global
// frame, or a footprint with poses or problems (`padding`: the clear record's, K8 has none).
struct Outlines {
  size_t count;
  const double* polygons;
  const double* footprint;
  uint32_t footprint_points, per_robot;
  const double* poses;
  const neo_mpc_problem* problems;
  double padding;
};
static Outlines outlines_of(const neo_mpc_stamp_batch& b) {
  return {b.count, b.polygons, b.footprint, b.footprint_points, b.per_robot_footprints, b.poses, b.problems, 0.0};
}
static Outlines outlines_of(const neo_mpc_fleet_clear& c) {
  return {c.count, c.polygons, c.footprint, c.footprint_points, c.per_robot_footprints, c.poses, c.problems, c.padding};
}

// Their shape: check_footprint_shape(), and behind each record's own refusals in between, this one
static int check_outline_pointers(const Outlines& o) {
  if (o.count > 0 && !o.polygons && (!o.footprint || (!o.poses && !o.problems)))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neither polygons nor a footprint with poses or problems");
  return NEO_MPC_OK;
}

// The host variants' staging, for o.count > 0: the values the device variants take as they come are looked at, then the
// host arrays go into the three buffers and `o` gets the device pointers -- of what the kernels read alone
static int stage_outlines(neo_mpc_handle* h, Outlines& o, DeviceBuffer& verts, DeviceBuffer& poses, DeviceBuffer& problems) {
  const size_t n = o.count, np = o.footprint_points;
  const double* v = o.polygons ? o.polygons : o.footprint;
  const size_t polygons = o.polygons || o.per_robot ? n : 1;
  if (int rc = check_vertices_finite(v, polygons, np, "vertex", "polygon")) return rc;
  if (!o.polygons) if (int rc = check_poses_finite(o.poses, o.problems, n)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const Outlines host = o;
  o.polygons = nullptr; o.footprint = nullptr; o.poses = nullptr; o.problems = nullptr;
  const double* d_verts = verts.upload(v, polygons * np * 16);
  if (!d_verts) return NEO_MPC_ERR_DEVICE;
  if (host.polygons) o.polygons = d_verts;
  else {
    o.footprint = d_verts;
    if (host.poses) o.poses = poses.upload(host.poses, n * 24);
    else o.problems = problems.upload(host.problems, n * sizeof(neo_mpc_problem));
    if (!o.poses && !o.problems) return NEO_MPC_ERR_DEVICE;
  }
  return NEO_MPC_OK;
}

// ---------------------------------------------------------------------------------------------- K8: the fleet stamp
// What both stamp entry points check: the record's shape and the handle's pool, never a value behind a pointer.
static int check_stamp_batch(const neo_mpc_handle* h, const neo_mpc_stamp_batch* b) {
  if (!h || !b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (b->reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_stamp_batch.reserved must be zero");
  if (int rc = check_footprint_shape(b->footprint_points, b->per_robot_footprints)) return rc;
  if (int rc = check_inflation_radii(b->inscribed_radius, b->inflation_radius, b->cost_scaling_factor)) return rc;
  if (int rc = check_outline_pointers(outlines_of(*b))) return rc;
  return check_pool_batch(h, b->count, b->inscribed_radius, b->inflation_radius, b->cost_scaling_factor);
}

// `o`: the outlines with device pointers, `b`: the radii.  Orders itself like roll(): it rewrites the device maps in place.
static int stamp(neo_mpc_handle* h, const neo_mpc_stamp_batch& b, const Outlines& o, void* stream) {
  const size_t n = o.count, np = o.footprint_points;
  // (every stamp ends a write of the fence)
  int rc = h->stamp_table.build(h->map.resolution, b.inscribed_radius, b.inflation_radius, b.cost_scaling_factor, h->fence);
  if (rc) return rc;
  // (no-ops from the second call with this count and footprint_points on)
  if ((rc = h->stamp_boxes.reserve(n * 32))) return rc;
  if (!o.polygons && (rc = h->stamp_polys.reserve(n * np * 16))) return rc;
  hipStream_t st = (hipStream_t)stream;
  // behind the ingest, roll or stamp that wrote the maps and every launch still reading them
  if ((rc = h->fence.begin_write(st))) return rc;
  StampArgs a;
  std::memset(&a, 0, sizeof(a));
  a.polygons = o.polygons;
  if (!o.polygons) { a.footprint = o.footprint; a.poses = o.poses; a.problems = o.poses ? nullptr : o.problems; }
  a.polys = h->stamp_polys.as<double>(); a.boxes = h->stamp_boxes.as<double>();
  a.table = h->stamp_table.buf.as<const uint8_t>();
  a.cells = const_cast<uint8_t*>(h->map.cells);   // (cell (0, 0) of the first map of map_buf, the handle's own)
  a.origins = h->map.pool_origins;
  a.res = h->map.resolution;
  a.stride = h->map.pool_stride;
  a.size_x = h->map.size_x; a.size_y = h->map.size_y; a.pitch = h->map.pitch;
  a.reach = h->stamp_table.reach;
  a.count = (uint32_t)n; a.points = o.footprint_points; a.per_robot = o.per_robot;
  launch_stamp(a, stream);
  HIP_TRY(hipGetLastError());
  return h->fence.end_write(st);   // a gate or solve behind it sees the stamped pool
}

// Both entry points: on `stream` with the record's device pointers, or from host arrays, synchronous
static int stamp_fleet(neo_mpc_handle* h, const neo_mpc_stamp_batch* b, bool on_device, void* stream) {
  int rc = check_stamp_batch(h, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  Outlines o = outlines_of(*b);
  if (on_device) HIP_TRY(hipSetDevice(h->device));
  else if ((rc = stage_outlines(h, o, h->verts, h->poses, h->problems))) return rc;
  rc = stamp(h, *b, o, stream);
  return on_device ? rc : finish_on_null_stream(rc);
}

int neo_mpc_stamp_fleet_device(neo_mpc_handle* h, const neo_mpc_stamp_batch* b, void* stream) { return stamp_fleet(h, b, true, stream); }

int neo_mpc_stamp_fleet(neo_mpc_handle* h, const neo_mpc_stamp_batch* b) { return stamp_fleet(h, b, false, nullptr); }

// ---------------------------------------------------------------------------------------------- K9: the world inflation
// What both inflation entry points refuse, before any HIP call
static int check_inflate_world_map(const neo_mpc_handle* h, double ins, double infl, double csf) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (int rc = check_inflation_radii(ins, infl, csf)) return rc;
  if (!h->world.has) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_world_map has not been called");
  return inflation_reach(h->world.resolution, ins, infl, csf, "the world map's ", nullptr);
}
// K9.  nav2's inflation layer on the handle's copy of the world map, in place (the contract: include/neo_mpc.h).  Orders
// itself like set_world_map's copy -- they write the same buffer -- on `stream`, or on the host and the null stream.
static int inflate_world_map(neo_mpc_handle* h, double ins, double infl, double csf, bool on_device, void* stream) {
  WorldMap& w = h->world;
  HIP_TRY(hipSetDevice(h->device));
  if (int rc = h->world_table.build(w.resolution, ins, infl, csf, w)) return rc;   // (every inflation records the world's event)
  hipStream_t st = (hipStream_t)stream;
  if (int rc = w.begin_write(h->fence, on_device, st)) return rc;
  h->world_scan.live_valid = false;   // (K12, as in set_world_map)
  InflateArgs a;
  std::memset(&a, 0, sizeof(a));
  a.world = w.buf.as<uint8_t>();
  a.table = h->world_table.buf.as<const uint8_t>();
  a.wsx = w.size_x; a.wsy = w.size_y;
  a.reach = h->world_table.reach;
  launch_inflate_world(a, stream);
  HIP_TRY(hipGetLastError());
  return w.end_write(st);   // a roll behind it, on whatever stream, cuts its windows from the inflated map
}

int neo_mpc_inflate_world_map_device(neo_mpc_handle* h, double ins, double infl, double csf, void* stream) {
  if (int rc = check_inflate_world_map(h, ins, infl, csf)) return rc;
  return inflate_world_map(h, ins, infl, csf, true, stream);
}

int neo_mpc_inflate_world_map(neo_mpc_handle* h, double ins, double infl, double csf) {
  if (int rc = check_inflate_world_map(h, ins, infl, csf)) return rc;
  return finish_on_null_stream(inflate_world_map(h, ins, infl, csf, false, nullptr));
}

// ---------------------------------------------------------------------------------------------- K10 to K14: the scan layers
// What the layer an update goes to is: the projection alone has none
enum Layer { kNoLayer, kPoolLayer, kWorldLayer };

// K12.  What a world-scan update refuses behind the record's own refusals, in place of check_pool_batch: the world map, the
// number of robots (free of the pool's), the reach at the world's resolution
static int check_world_scan(const neo_mpc_handle* h, size_t count, double ins, double infl, double csf) {
  if (!h->world.has) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_world_map has not been called");
  if (count > NEO_MPC_MAX_POOL_MAPS) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "%zu robots: at most %u per call", count, NEO_MPC_MAX_POOL_MAPS);
  return inflation_reach(h->world.resolution, ins, infl, csf, "the world map's ", nullptr);
}

static int check_unknown_value(uint32_t u) {
  return u == 0 || u == 255 ? NEO_MPC_OK : fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown_value %u is neither 0 nor 255", u);
}

// What an update refuses of its settings and its target, behind the refusals of the record it came in: the four ranges, the
// radii, then the pool's refusals or the world's.  `s`: the update's record, of points (K10, K12) or made of a laser record's
// fields (scan_batch_of)
static int check_update_target(const neo_mpc_handle* h, const neo_mpc_scan_batch& s, Layer layer) {
  for (const double r : {s.obstacle_max_range, s.obstacle_min_range, s.raytrace_max_range, s.raytrace_min_range})
    if (!std::isfinite(r) || r < 0.0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "range %g must be finite and not negative", r);
  if (int rc = check_inflation_radii(s.inscribed_radius, s.inflation_radius, s.cost_scaling_factor)) return rc;
  if (layer == kWorldLayer) return check_world_scan(h, s.count, s.inscribed_radius, s.inflation_radius, s.cost_scaling_factor);
  return check_pool_batch(h, s.count, s.inscribed_radius, s.inflation_radius, s.cost_scaling_factor);
}

// K10, K12.  What the update entry points check: the record's shape and the handle's pool -- or its world map --,
// never a value behind a pointer.
static int check_scan_batch(const neo_mpc_handle* h, const neo_mpc_scan_batch* b, Layer layer) {
  if (!h || !b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (b->reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_scan_batch.reserved must be zero");
  if (b->flags & ~(NEO_MPC_SCAN_CLEAR | NEO_MPC_SCAN_MARK)) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", b->flags);
  if (int rc = check_unknown_value(b->unknown_value)) return rc;
  if (b->max_points > NEO_MPC_MAX_SCAN_POINTS)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "max_points %u: at most %u", b->max_points, NEO_MPC_MAX_SCAN_POINTS);
  if (b->flags != 0 && b->count > 0 && (!b->points || !b->sensor_origins))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "points and sensor_origins must not be null with flags 0x%x", b->flags);
  return check_update_target(h, *b, layer);
}

// K12.  What the update entry points check of the clear record (null: none): its shape, never a value behind a pointer
static int check_fleet_clear(const neo_mpc_fleet_clear* c, size_t count) {
  if (!c) return NEO_MPC_OK;
  if (c->reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_fleet_clear.reserved must be zero");
  if (int rc = check_footprint_shape(c->footprint_points, c->per_robot_footprints)) return rc;
  if (!std::isfinite(c->padding) || c->padding < 0.0)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "padding %g must be finite and not negative", c->padding);
  if (c->count != count)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "%zu outlines for %zu robots: they are one to one", c->count, count);
  return check_outline_pointers(outlines_of(*c));
}

// The rays of an update as K10's and K12's kernels take them.  `d`: the record with device pointers; `laser`: K11's
// projection of `sources` scanners a robot into d.points and d.sensor_origins
static void fill_rays(ScanArgs& s, const neo_mpc_scan_batch& d, const InflationTable& table, const LaserArgs* laser) {
  if (d.flags != 0) { s.points = d.points; s.point_counts = d.point_counts; s.sensor_origins = d.sensor_origins; }
  s.table = table.buf.as<const uint8_t>();
  s.obstacle_max = d.obstacle_max_range; s.obstacle_min = d.obstacle_min_range;
  s.raytrace_max = d.raytrace_max_range; s.raytrace_min = d.raytrace_min_range;
  s.reach = table.reach;
  s.count = (uint32_t)d.count; s.max_points = d.max_points; s.flags = d.flags; s.unknown = d.unknown_value;
  // (without K11 every point of a robot is its one source's: the address arithmetic of one observation per robot)
  s.sources = laser ? laser->sources : 1u;
  s.points_per_source = laser ? laser->beams : (d.max_points > 0 ? d.max_points : 1u);
}

// K10.  `d`: the record with device pointers.  Orders itself like stamp(): it rewrites the device maps in place, and the layer
// buffers inside the same write.  `laser`: K11's projection, enqueued inside the same write, in front of the layers' launches
// (the rays of the previous update, which read the handle's own points, lie behind the previous write's end).
static int scan(neo_mpc_handle* h, const neo_mpc_scan_batch& d, void* stream, const LaserArgs* laser = nullptr) {
  const DevMap& m = h->map;
  ScanLayers& l = h->scan;
  // (every update ends a write of the fence)
  int rc = l.table.build(m.resolution, d.inscribed_radius, d.inflation_radius, d.cost_scaling_factor, h->fence);
  if (rc) return rc;
  const bool same = l.matches(m, d.unknown_value);
  if (!same && (rc = l.resize(m, d.unknown_value))) return rc;   // (d.count is the pool's: check_pool_batch)
  hipStream_t st = (hipStream_t)stream;
  if ((rc = h->fence.begin_write(st))) return rc;
  ScanArgs a;
  std::memset(&a, 0, sizeof(a));
  fill_rays(a, d, l.table, laser);
  a.layer = l.layer.as<uint8_t>(); a.work = l.work.as<uint8_t>(); a.layer_origins = l.origins.as<double>();
  a.cells = const_cast<uint8_t*>(m.cells);   // (cell (0, 0) of the first map of map_buf, the handle's own)
  a.origins = m.pool_origins;
  a.res = m.resolution;
  a.stride = m.pool_stride; a.layer_stride = (int64_t)l.stride();
  a.size_x = m.size_x; a.size_y = m.size_y; a.pitch = m.pitch; a.layer_pitch = l.pitch();
  a.reset = same ? 0u : 1u;
  if (laser) launch_laser_project(*laser, stream);
  launch_scan_layer(a, stream);
  HIP_TRY(hipGetLastError());
  if ((rc = h->fence.end_write(st))) return rc;   // a stamp, gate or solve behind it sees the windows with the layer in them
  l.adopt();
  return NEO_MPC_OK;
}

// K12 to K14.  `d`, `c`: the record and the outlines to clear with device pointers (`c` may be null).  Orders itself like
// inflate_world_map(): it reads the world map and rewrites what the roll reads -- on `stream`, or on the host and the null
// stream.  `laser`: as scan()'s, in front of the rays.
static int world_scan(neo_mpc_handle* h, const neo_mpc_scan_batch& d, const Outlines* c, bool on_device, void* stream,
                      const LaserArgs* laser = nullptr) {
  WorldMap& w = h->world;
  WorldScanLayer& l = h->world_scan;
  int rc = l.table.build(w.resolution, d.inscribed_radius, d.inflation_radius, d.cost_scaling_factor, w);   // (every update records the world's event)
  if (rc) return rc;
  const bool same = l.matches(w, d.unknown_value);
  if (!same && (rc = l.resize(w, d.unknown_value))) return rc;
  if ((rc = l.reserve_denoised()) || (rc = l.reserve_decay())) return rc;
  hipStream_t st = (hipStream_t)stream;
  // behind the last roll, which reads `live` or the world map, and the previous copy, inflation or update
  if ((rc = w.begin_write(h->fence, on_device, st))) return rc;
  WorldScanArgs a;
  std::memset(&a, 0, sizeof(a));
  fill_rays(a.s, d, l.table, laser);
  a.s.res = w.resolution;
  a.layer = l.layer.as<uint8_t>(); a.world = w.buf.as<const uint8_t>(); a.live = l.live.as<uint8_t>();
  if (c && c->count > 0) {
    a.polygons = c->polygons;
    if (!c->polygons) { a.footprint = c->footprint; a.poses = c->poses; a.problems = c->poses ? nullptr : c->problems; }
    a.padding = c->padding; a.points = c->footprint_points; a.per_robot = c->per_robot; a.clear = 1u;
  }
  a.wres = w.resolution; a.wox = w.origin_x; a.woy = w.origin_y;
  a.wsx = w.size_x; a.wsy = w.size_y;
  a.reset = same ? 0u : 1u;
  if (l.group >= 2) { a.denoised = l.denoised.as<uint8_t>(); a.group = l.group; a.connectivity = l.connectivity; }
  if (l.max_age != 0) {
    a.stamp = l.stamp.as<uint32_t>(); a.clock = l.clock.as<uint32_t>(); a.max_age = l.max_age;
    a.stamp_fresh = l.decaying ? 0u : 1u;   // (the marks that are there count as made by the last scan update before this one)
  }
  if (laser) launch_laser_project(*laser, stream);
  launch_world_scan(a, stream);
  HIP_TRY(hipGetLastError());
  if ((rc = w.end_write(st))) return rc;   // a roll behind it, on whatever stream, cuts its windows from `live`
  l.valid = true; l.live_valid = true;
  l.filtered = a.group >= 2;
  l.decaying = a.max_age != 0;
  return NEO_MPC_OK;
}

// The host variants' staging of an observation (K10, K12): the values the device variants take as they come are looked at,
// then the arrays go into ScanLayers' staging and `d` gets the device pointers
static int stage_observation(neo_mpc_handle* h, const neo_mpc_scan_batch* b, neo_mpc_scan_batch& d) {
  const size_t n = b->count;
  d.points = nullptr; d.point_counts = nullptr; d.sensor_origins = nullptr;
  if (b->flags != 0) {
    for (size_t k = 0; k < n; ++k) {
      if (b->point_counts && b->point_counts[k] > b->max_points)
        return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "point_counts[%zu] = %u is more than max_points %u", k, b->point_counts[k], b->max_points);
      if (!std::isfinite(b->sensor_origins[2 * k]) || !std::isfinite(b->sensor_origins[2 * k + 1]))
        return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "the sensor origin of robot %zu is not finite", k);
    }
  }
  HIP_TRY(hipSetDevice(h->device));
  if (b->flags != 0) {
    if (!(d.sensor_origins = h->scan.sensors.upload(b->sensor_origins, n * 16))) return NEO_MPC_ERR_DEVICE;
    if (b->max_points > 0 && !(d.points = h->scan.points.upload(b->points, n * b->max_points * 16))) return NEO_MPC_ERR_DEVICE;
    if (b->point_counts && !(d.point_counts = h->scan.point_counts.upload(b->point_counts, n * 4))) return NEO_MPC_ERR_DEVICE;
  }
  return NEO_MPC_OK;
}

// The update entry points from points: K10 (`layer` the pool's, `c` null) and K12, on `stream` with the records' device
// pointers, or from host arrays, synchronous.  The refusals in this order: the record's shape, the clear record's, then --
// behind `count == 0`, which is no work -- the observation's values and the clear record's.
static int update_from_points(neo_mpc_handle* h, const neo_mpc_scan_batch* b, const neo_mpc_fleet_clear* c, Layer layer,
                              bool on_device, void* stream) {
  int rc = check_scan_batch(h, b, layer);
  if (rc || (rc = check_fleet_clear(c, b->count))) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  neo_mpc_scan_batch d = *b;
  Outlines clear{};
  if (c) clear = outlines_of(*c);
  if (on_device) HIP_TRY(hipSetDevice(h->device));
  else {
    WorldScanLayer& l = h->world_scan;
    if ((rc = stage_observation(h, b, d))) return rc;
    if (clear.count > 0 && (rc = stage_outlines(h, clear, l.verts, l.poses, l.problems))) return rc;
  }
  rc = layer == kWorldLayer ? world_scan(h, d, &clear, on_device, stream) : scan(h, d, stream);
  return on_device ? rc : finish_on_null_stream(rc);
}

int neo_mpc_update_scan_layer_device(neo_mpc_handle* h, const neo_mpc_scan_batch* b, void* stream) {
  return update_from_points(h, b, nullptr, kPoolLayer, true, stream);
}
int neo_mpc_update_scan_layer(neo_mpc_handle* h, const neo_mpc_scan_batch* b) {
  return update_from_points(h, b, nullptr, kPoolLayer, false, nullptr);
}
int neo_mpc_update_world_scan_layer_device(neo_mpc_handle* h, const neo_mpc_scan_batch* b, const neo_mpc_fleet_clear* c, void* stream) {
  return update_from_points(h, b, c, kWorldLayer, true, stream);
}
int neo_mpc_update_world_scan_layer(neo_mpc_handle* h, const neo_mpc_scan_batch* b, const neo_mpc_fleet_clear* c) {
  return update_from_points(h, b, c, kWorldLayer, false, nullptr);
}

// ---------------------------------------------------------------------------------------------- K11: from LaserScan ranges
// What the projection refuses of one scanner
static int check_scanner(const neo_mpc_scanner& sc, uint32_t s) {
  if (sc.reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_scanner.reserved of scanner %u must be zero", s);
  if (sc.flags & ~NEO_MPC_LASER_INF_IS_VALID) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown flags 0x%x of scanner %u", sc.flags, s);
  for (const double v : {sc.mount_x, sc.mount_y, sc.mount_yaw, sc.angle_min, sc.angle_increment, sc.range_min, sc.range_max})
    if (!std::isfinite(v)) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "a mount, angle or range of scanner %u is not finite", s);
  if (sc.range_min < 0.0 || sc.range_max < sc.range_min)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "scanner %u: range_min %g, range_max %g", s, sc.range_min, sc.range_max);
  return NEO_MPC_OK;
}

// The update's record for a laser record's settings and the points projected from it
static neo_mpc_scan_batch scan_batch_of(const neo_mpc_laser_batch& d, const double* points = nullptr, const double* origins = nullptr) {
  neo_mpc_scan_batch sb;
  std::memset(&sb, 0, sizeof(sb));
  sb.count = d.count; sb.points = points; sb.sensor_origins = origins;
  sb.max_points = d.sources * d.beams; sb.flags = d.scan_flags;
  sb.obstacle_max_range = d.obstacle_max_range; sb.obstacle_min_range = d.obstacle_min_range;
  sb.raytrace_max_range = d.raytrace_max_range; sb.raytrace_min_range = d.raytrace_min_range;
  sb.inscribed_radius = d.inscribed_radius; sb.inflation_radius = d.inflation_radius; sb.cost_scaling_factor = d.cost_scaling_factor;
  sb.unknown_value = d.unknown_value;
  return sb;
}

// What the six entry points check: the record's shape, the scanners (host configuration) and, for an update, what
// check_scan_batch checks of the handle's pool or world map -- never a value behind ranges, poses or the out pointers.
static int check_laser_batch(const neo_mpc_handle* h, const neo_mpc_laser_batch* b, Layer layer, bool device) {
  const bool update = layer != kNoLayer;
  if (!h || !b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (b->reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_laser_batch.reserved must be zero");
  if (b->sources < 1 || b->sources > NEO_MPC_MAX_SCAN_SOURCES)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "sources %u outside [1, %u]", b->sources, NEO_MPC_MAX_SCAN_SOURCES);
  if (b->beams < 1 || b->beams > NEO_MPC_MAX_SCAN_POINTS / b->sources)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "beams %u: at least 1, and with %u sources at most %u points", b->beams, b->sources, NEO_MPC_MAX_SCAN_POINTS);
  if (!b->scanners) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "scanners must not be null");
  if (b->count > 0 && (!b->ranges || !b->poses)) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "ranges and poses must not be null");
  if (!update && b->count > 0 && (!b->points_out || !b->origins_out))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "points_out and origins_out must not be null");
  if (device && ((uintptr_t)b->points_out & 15)) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "points_out is not 16-byte aligned");
  if (update) {
    if (b->scan_flags == 0 || (b->scan_flags & ~(NEO_MPC_SCAN_CLEAR | NEO_MPC_SCAN_MARK)))
      return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "scan_flags 0x%x: NEO_MPC_SCAN_CLEAR, NEO_MPC_SCAN_MARK or both", b->scan_flags);
    if (int rc = check_unknown_value(b->unknown_value)) return rc;
  }
  for (uint32_t s = 0; s < b->sources; ++s)
    if (int rc = check_scanner(b->scanners[s], s)) return rc;
  return update ? check_update_target(h, scan_batch_of(*b), layer) : NEO_MPC_OK;
}

// `d`: the record with device pointers (points_out / origins_out null: the handle's own) -> the kernel's arguments, the beam
// tables and the handle's buffers in place
static int laser_args(neo_mpc_handle* h, const neo_mpc_laser_batch& d, LaserArgs& a) {
  LaserProjection& l = h->laser;
  if (int rc = l.build(d.scanners, d.sources, d.beams)) return rc;
  if (int rc = l.reserve_out(d.count, d.sources, d.beams, !d.points_out, !d.origins_out)) return rc;
  std::memset(&a, 0, sizeof(a));
  a.ranges = d.ranges; a.poses = d.poses;
  a.table = l.table.as<const double>();
  a.points = d.points_out ? d.points_out : l.points.as<double>();
  a.origins = d.origins_out ? d.origins_out : l.origins.as<double>();
  for (uint32_t s = 0; s < d.sources; ++s) {
    const neo_mpc_scanner& sc = d.scanners[s];
    LaserSource& o = a.source[s];
    o.mount_x = sc.mount_x; o.mount_y = sc.mount_y; o.range_min = sc.range_min; o.range_max = sc.range_max;
    o.inf_range = sc.range_max - 1e-4;
    o.inf_is_valid = sc.flags & NEO_MPC_LASER_INF_IS_VALID;
  }
  a.count = (uint32_t)d.count; a.sources = d.sources; a.beams = d.beams;
  return NEO_MPC_OK;
}

// The projection -- alone it touches neither maps nor layers, so it is in order on its stream and nothing else -- or the
// projection and the layer's update over all sources, in one write of what the update rewrites
static int project(neo_mpc_handle* h, const neo_mpc_laser_batch& d, const Outlines* c, Layer layer, bool on_device, void* stream) {
  LaserArgs a;
  if (int rc = laser_args(h, d, a)) return rc;
  if (layer == kNoLayer) {
    launch_laser_project(a, stream);
    HIP_TRY(hipGetLastError());
    return NEO_MPC_OK;
  }
  const neo_mpc_scan_batch sb = scan_batch_of(d, a.points, a.origins);
  return layer == kWorldLayer ? world_scan(h, sb, c, on_device, stream, &a) : scan(h, sb, stream, &a);
}

// The host variants' staging of ranges: the poses are looked at, ranges and poses go into the handle's staging, and the
// projection goes into the handle's own buffers ...
static int stage_ranges(neo_mpc_handle* h, const neo_mpc_laser_batch* b, neo_mpc_laser_batch& d) {
  const size_t n = b->count;
  if (int rc = check_poses_finite(b->poses, nullptr, n)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  d.points_out = nullptr; d.origins_out = nullptr;
  if (!(d.ranges = h->laser.ranges.upload(b->ranges, n * b->sources * b->beams * 4))) return NEO_MPC_ERR_DEVICE;
  if (!(d.poses = h->poses.upload(b->poses, n * 24))) return NEO_MPC_ERR_DEVICE;
  return NEO_MPC_OK;
}
// ... which are read back where asked for, behind the wait for the null stream
static int read_back_projection(neo_mpc_handle* h, const neo_mpc_laser_batch* b) {
  const size_t scans = b->count * b->sources;
  if (b->points_out) HIP_TRY(hipMemcpy(b->points_out, h->laser.points.ptr, scans * b->beams * 16, hipMemcpyDeviceToHost));
  if (b->origins_out) HIP_TRY(hipMemcpy(b->origins_out, h->laser.origins.ptr, scans * 16, hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

// The entry points from ranges: the projection alone (kNoLayer), K10's update and K12's (`c`: its clear record), on `stream`
// with the records' device pointers, or from host arrays, synchronous.  The refusals in update_from_points' order.
static int from_ranges(neo_mpc_handle* h, const neo_mpc_laser_batch* b, const neo_mpc_fleet_clear* c, Layer layer, bool on_device,
                       void* stream) {
  int rc = check_laser_batch(h, b, layer, on_device);
  if (rc || (rc = check_fleet_clear(c, b->count))) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  neo_mpc_laser_batch d = *b;
  Outlines clear{};
  if (c) clear = outlines_of(*c);
  if (on_device) {
    HIP_TRY(hipSetDevice(h->device));
    return project(h, d, &clear, layer, true, stream);
  }
  WorldScanLayer& l = h->world_scan;
  if ((rc = stage_ranges(h, b, d))) return rc;
  if (clear.count > 0 && (rc = stage_outlines(h, clear, l.verts, l.poses, l.problems))) return rc;
  if ((rc = finish_on_null_stream(project(h, d, &clear, layer, false, nullptr)))) return rc;
  return read_back_projection(h, b);
}

int neo_mpc_laser_beam_table(const neo_mpc_scanner* scanner, uint32_t beams, double* table_out) {
  if (!scanner || !table_out) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (beams < 1 || beams > NEO_MPC_MAX_SCAN_POINTS) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "beams %u outside [1, %u]", beams, NEO_MPC_MAX_SCAN_POINTS);
  if (int rc = check_scanner(*scanner, 0)) return rc;
  laser_beam_table(*scanner, beams, table_out);
  return NEO_MPC_OK;
}

int neo_mpc_project_laser_device(neo_mpc_handle* h, const neo_mpc_laser_batch* b, void* stream) {
  return from_ranges(h, b, nullptr, kNoLayer, true, stream);
}
int neo_mpc_project_laser(neo_mpc_handle* h, const neo_mpc_laser_batch* b) { return from_ranges(h, b, nullptr, kNoLayer, false, nullptr); }
int neo_mpc_update_scan_layer_from_ranges_device(neo_mpc_handle* h, const neo_mpc_laser_batch* b, void* stream) {
  return from_ranges(h, b, nullptr, kPoolLayer, true, stream);
}
int neo_mpc_update_scan_layer_from_ranges(neo_mpc_handle* h, const neo_mpc_laser_batch* b) {
  return from_ranges(h, b, nullptr, kPoolLayer, false, nullptr);
}
int neo_mpc_update_world_scan_layer_from_ranges_device(neo_mpc_handle* h, const neo_mpc_laser_batch* b, const neo_mpc_fleet_clear* c,
                                                       void* stream) {
  return from_ranges(h, b, c, kWorldLayer, true, stream);
}
int neo_mpc_update_world_scan_layer_from_ranges(neo_mpc_handle* h, const neo_mpc_laser_batch* b, const neo_mpc_fleet_clear* c) {
  return from_ranges(h, b, c, kWorldLayer, false, nullptr);
}

// ---------------------------------------------------------------------------------------------- the layers read back, reset, K13's and K14's settings
int neo_mpc_get_scan_layer(neo_mpc_handle* h, uint32_t first, uint32_t count, uint8_t* cells_out, double* origins_out) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  const ScanLayers& l = h->scan;
  if (!l.valid) return fail(NEO_MPC_ERR_NO_COSTMAP, "no scan layer: neo_mpc_update_scan_layer has not been called since the last reset");
  const uint32_t maps = (uint32_t)l.count;
  if (first > maps || count > maps - first)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "layers [%u, %u + %u) outside the %u there are", first, first, count, maps);
  if (count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  int rc = h->fence.wait_writer_host();   // the update in flight
  if (rc) return rc;
  if ((rc = download_maps(l.layer.as<uint8_t>(), l.pitch(), l.stride(), l.size_x, l.size_y, first, count, cells_out))) return rc;
  if (origins_out)
    HIP_TRY(hipMemcpy(origins_out, l.origins.as<double>() + 2 * (size_t)first, (size_t)count * 16, hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

int neo_mpc_reset_scan_layer(neo_mpc_handle* h) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  h->scan.valid = false;
  return NEO_MPC_OK;
}

int neo_mpc_get_world_scan_layer(neo_mpc_handle* h, uint8_t* layer_out, uint8_t* live_out) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  WorldScanLayer& l = h->world_scan;
  if (!l.valid)
    return fail(NEO_MPC_ERR_NO_COSTMAP, "no world scan layer: neo_mpc_update_world_scan_layer has not been called since the last reset");
  if (!layer_out && !live_out) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (int rc = h->world.wait_writer_host()) return rc;   // the update in flight
  if (layer_out) HIP_TRY(hipMemcpy(layer_out, l.layer.ptr, l.bytes(), hipMemcpyDeviceToHost));
  if (live_out) HIP_TRY(hipMemcpy(live_out, l.live.ptr, l.bytes(), hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

int neo_mpc_set_world_scan_denoise(neo_mpc_handle* h, uint32_t minimal_group_size, uint32_t connectivity) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (minimal_group_size > NEO_MPC_MAX_DENOISE_GROUP)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "minimal_group_size %u is more than NEO_MPC_MAX_DENOISE_GROUP %u", minimal_group_size,
                NEO_MPC_MAX_DENOISE_GROUP);
  if (connectivity != 4 && connectivity != 8) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "connectivity %u is neither 4 nor 8", connectivity);
  h->world_scan.group = minimal_group_size >= 2 ? minimal_group_size : 0u;   // (the next update allocates D and filters)
  h->world_scan.connectivity = connectivity;
  return NEO_MPC_OK;
}

int neo_mpc_get_world_scan_denoised(neo_mpc_handle* h, uint8_t* cells_out) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  WorldScanLayer& l = h->world_scan;
  if (!l.valid)
    return fail(NEO_MPC_ERR_NO_COSTMAP, "no world scan layer: neo_mpc_update_world_scan_layer has not been called since the last reset");
  if (!cells_out) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (int rc = h->world.wait_writer_host()) return rc;   // the update in flight
  HIP_TRY(hipMemcpy(cells_out, l.filtered ? l.denoised.ptr : l.layer.ptr, l.bytes(), hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

int neo_mpc_set_world_scan_decay(neo_mpc_handle* h, uint32_t max_age) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  h->world_scan.max_age = max_age;   // (the next update allocates the stamps and the clock, and lets marks expire)
  return NEO_MPC_OK;
}

int neo_mpc_get_world_scan_ages(neo_mpc_handle* h, uint32_t* ages_out) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  WorldScanLayer& l = h->world_scan;
  if (!l.valid)
    return fail(NEO_MPC_ERR_NO_COSTMAP, "no world scan layer: neo_mpc_update_world_scan_layer has not been called since the last reset");
  if (!l.decaying)
    return fail(NEO_MPC_ERR_UNSUPPORTED, "no ages: the last update ran without decay (neo_mpc_set_world_scan_decay)");
  if (!ages_out) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (int rc = h->world.wait_writer_host()) return rc;   // the update in flight
  // the stamps go where the ages will be, and become ages under the layer's marks
  std::vector<uint8_t> layer(l.bytes());
  uint32_t now = 0;
  HIP_TRY(hipMemcpy(ages_out, l.stamp.ptr, l.bytes() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(layer.data(), l.layer.ptr, l.bytes(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&now, l.clock.ptr, sizeof(now), hipMemcpyDeviceToHost));
  for (size_t at = 0; at < layer.size(); ++at) ages_out[at] = layer[at] == 254 ? now - ages_out[at] : NEO_MPC_NO_AGE;
  return NEO_MPC_OK;
}

int neo_mpc_reset_world_scan_layer(neo_mpc_handle* h) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  h->world_scan.valid = false;
  h->world_scan.live_valid = false;
  return NEO_MPC_OK;
}

// ---------------------------------------------------------------------------------------------- K15: the plan check
// What both entry points check: the record's shape, never a value behind a pointer.
static int check_plan_check_batch(const neo_mpc_handle* h, const neo_mpc_plan_check_batch* b) {
  if (!h || !b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->world.has) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_world_map has not been called");
  if (b->reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_plan_check_batch.reserved must be zero (got %u)", b->reserved);
  if (b->max_cost < 1 || b->max_cost > 254) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "max_cost %u outside [1, 254]", b->max_cost);
  if (b->unknown_blocks > 1) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown_blocks must be 0 or 1 (got %u)", b->unknown_blocks);
  if (b->outside_value > 255) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "outside_value %u is no cell value (0 .. 255)", b->outside_value);
  if ((b->footprint == nullptr) != (b->footprint_points == 0))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "footprint and footprint_points (%u) must be given together", b->footprint_points);
  if (b->footprint)
    if (int rc = check_footprint_shape(b->footprint_points, 0)) return rc;
  if (b->count > 0 && (!b->plan_poses || !b->plan_offsets || !b->results))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "plan_poses/plan_offsets/results must not be null");
  return check_count(b->count);
}

// `d`: the record with device pointers.  Orders itself like roll(), whose reads it shares -- the map the next roll would cut
// its windows from, behind that map's writer -- and like a roll it runs between the fence's begin_write and end_write: every
// rewrite of the world map waits for the fence's last write (WorldMap::begin_write), and that is how it waits for this read.
static int plan_check(neo_mpc_handle* h, const neo_mpc_plan_check_batch& d, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = h->fence.begin_write(st))) return rc;
  if ((rc = h->world.wait_writer(st))) return rc;
  const WorldMap& w = h->world;
  PlanCheckArgs a;
  std::memset(&a, 0, sizeof(a));
  a.plan_poses = d.plan_poses; a.plan_offsets = d.plan_offsets; a.robot_poses = d.robot_poses; a.footprint = d.footprint;
  a.results = d.results;
  // (K12: while an update's composition is current it is the map -- roll()'s choice, same geometry, same event)
  a.world = h->world_scan.live_valid ? h->world_scan.live.as<const uint8_t>() : w.buf.as<const uint8_t>();
  a.wres = w.resolution; a.winv = 1.0 / w.resolution; a.wox = w.origin_x; a.woy = w.origin_y;
  a.wsx = w.size_x; a.wsy = w.size_y;
  a.count = (uint32_t)d.count; a.footprint_points = d.footprint_points;
  a.max_cost = d.max_cost; a.unknown_blocks = d.unknown_blocks; a.outside = d.outside_value; a.max_poses = d.max_poses;
  launch_plan_check(a, stream);
  HIP_TRY(hipGetLastError());
  return h->fence.end_write(st);
}

int neo_mpc_check_plans_device(neo_mpc_handle* h, const neo_mpc_plan_check_batch* b, void* stream) {
  int rc = check_plan_check_batch(h, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  return plan_check(h, *b, stream);
}

int neo_mpc_check_plans(neo_mpc_handle* h, const neo_mpc_plan_check_batch* b) {
  int rc = check_plan_check_batch(h, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  const size_t n = b->count, np = b->footprint_points;
  // the values the device variant takes as they come are looked at here
  for (size_t i = 0; i < n; ++i)
    if (b->plan_offsets[i + 1] < b->plan_offsets[i])
      return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "plan_offsets[%zu] = %u is below plan_offsets[%zu] = %u", i + 1, b->plan_offsets[i + 1],
                  i, b->plan_offsets[i]);
  if (b->footprint && (rc = check_vertices_finite(b->footprint, 1, np, "footprint vertex", "polygon"))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t total = b->plan_offsets[n];
  if ((rc = h->plan_poses.reserve(total * 24 + 8))) return rc;   // (never empty: a fleet without a plan pose stages nothing)
  if ((rc = h->plan_checks.reserve(n * sizeof(neo_mpc_plan_check)))) return rc;
  neo_mpc_plan_check_batch d = *b;
  d.results = h->plan_checks.as<neo_mpc_plan_check>();
  if (!(d.plan_poses = h->plan_poses.upload(b->plan_poses, total * 24))) return NEO_MPC_ERR_DEVICE;
  if (!(d.plan_offsets = h->plan_offsets.upload(b->plan_offsets, (n + 1) * 4))) return NEO_MPC_ERR_DEVICE;
  if (b->robot_poses && !(d.robot_poses = h->poses.upload(b->robot_poses, n * 24))) return NEO_MPC_ERR_DEVICE;
  if (b->footprint && !(d.footprint = h->verts.upload(b->footprint, np * 16))) return NEO_MPC_ERR_DEVICE;
  if ((rc = plan_check(h, d, nullptr))) return finish_on_null_stream(rc);
  // (a blocking copy on the null stream, behind the kernel)
  HIP_TRY(hipMemcpy(b->results, h->plan_checks.ptr, n * sizeof(neo_mpc_plan_check), hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

// ---------------------------------------------------------------------------------------------- K16: the grid planner
// What both entry points check: the record's shape, never a value behind a pointer.
static int check_replan_batch(const neo_mpc_handle* h, const neo_mpc_replan_batch* b) {
  if (!h || !b) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->world.has) return fail(NEO_MPC_ERR_NO_COSTMAP, "neo_mpc_set_world_map has not been called");
  if (b->reserved != 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neo_mpc_replan_batch.reserved must be zero (got %u)", b->reserved);
  if (b->window < 4 || b->window > 128) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "window %u outside [4, 128]", b->window);
  if (b->max_cost < 1 || b->max_cost > 254) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "max_cost %u outside [1, 254]", b->max_cost);
  if (b->unknown_cost > 252) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "unknown_cost %u outside [0, 252]", b->unknown_cost);
  if (b->neutral_cost < 1 || b->neutral_cost > 255)
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "neutral_cost %u outside [1, 255]", b->neutral_cost);
  if (b->max_path_cells == 0) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "max_path_cells must be at least 1");
  if (b->count > 0 && (!b->starts || !b->goals || !b->path_cells || !b->results))
    return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "starts/goals/path_cells/results must not be null");
  return check_count(b->count);
}

// `d`: the record with device pointers.  Ordered exactly like plan_check(), whose map it reads.
static int replan(neo_mpc_handle* h, const neo_mpc_replan_batch& d, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = h->fence.begin_write(st))) return rc;
  if ((rc = h->world.wait_writer(st))) return rc;
  const WorldMap& w = h->world;
  ReplanArgs a;
  std::memset(&a, 0, sizeof(a));
  a.starts = d.starts; a.goals = d.goals; a.checks = d.checks;
  a.path_cells = d.path_cells; a.path_poses = d.path_poses; a.results = d.results;
  a.world = h->world_scan.live_valid ? h->world_scan.live.as<const uint8_t>() : w.buf.as<const uint8_t>();
  a.wres = w.resolution; a.winv = 1.0 / w.resolution; a.wox = w.origin_x; a.woy = w.origin_y;
  a.wsx = w.size_x; a.wsy = w.size_y;
  a.count = (uint32_t)d.count; a.window = d.window;
  a.max_cost = d.max_cost; a.unknown_cost = d.unknown_cost; a.neutral_cost = d.neutral_cost; a.max_path_cells = d.max_path_cells;
  launch_replan(a, stream);
  HIP_TRY(hipGetLastError());
  return h->fence.end_write(st);
}

int neo_mpc_replan_plans_device(neo_mpc_handle* h, const neo_mpc_replan_batch* b, void* stream) {
  int rc = check_replan_batch(h, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  return replan(h, *b, stream);
}

int neo_mpc_replan_plans(neo_mpc_handle* h, const neo_mpc_replan_batch* b) {
  int rc = check_replan_batch(h, b);
  if (rc) return rc;
  if (b->count == 0) return NEO_MPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = b->count, cells_bytes = n * b->max_path_cells * 8, poses_bytes = n * b->max_path_cells * 24;
  // staged through the buffers of the other synchronous plan calls (K4's and K15's host variants: all of them on the null
  // stream, each finished when it returns): starts and goals in `poses` and `verts`, the mask in `plan_checks`, the records in
  // `carrots`, the paths in `plan_offsets` and `plan_poses` -- the handle holds nothing of K16's own
  DeviceBuffer &results = h->carrots, &cells = h->plan_offsets, &poses = h->plan_poses;
  if ((rc = results.reserve(n * sizeof(neo_mpc_replan)))) return rc;
  neo_mpc_replan_batch d = *b;
  d.results = results.as<neo_mpc_replan>();
  if (!(d.starts = h->poses.upload(b->starts, n * 16))) return NEO_MPC_ERR_DEVICE;
  if (!(d.goals = h->verts.upload(b->goals, n * 16))) return NEO_MPC_ERR_DEVICE;
  if (b->checks && !(d.checks = h->plan_checks.upload(b->checks, n * sizeof(neo_mpc_plan_check)))) return NEO_MPC_ERR_DEVICE;
  // the paths go up before they come back: what the kernel does not write keeps the caller's values
  if (!(d.path_cells = cells.upload(b->path_cells, cells_bytes))) return NEO_MPC_ERR_DEVICE;
  if (b->path_poses && !(d.path_poses = poses.upload(b->path_poses, poses_bytes))) return NEO_MPC_ERR_DEVICE;
  if ((rc = replan(h, d, nullptr))) return finish_on_null_stream(rc);
  // (blocking copies on the null stream, behind the kernel)
  HIP_TRY(hipMemcpy(b->results, results.ptr, n * sizeof(neo_mpc_replan), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b->path_cells, cells.ptr, cells_bytes, hipMemcpyDeviceToHost));
  if (b->path_poses) HIP_TRY(hipMemcpy(b->path_poses, poses.ptr, poses_bytes, hipMemcpyDeviceToHost));
  return NEO_MPC_OK;
}

int neo_mpc_kernel_info(const neo_mpc_handle* h, uint32_t* lds_bytes, uint32_t* reach_cells, uint32_t* tile_in_lds) {
  if (!h) return fail(NEO_MPC_ERR_INVALID_ARGUMENT, "null handle");
  if (lds_bytes) *lds_bytes = (uint32_t)h->lds.total_bytes;
  if (reach_cells) *reach_cells = (uint32_t)h->lds.reach;
  if (tile_in_lds) *tile_in_lds = h->lds.tile_w ? 1u : 0u;
  return NEO_MPC_OK;
}

}  // extern "C"
