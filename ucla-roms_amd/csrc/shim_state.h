// shim_state.h -- what the C-ABI modules outside roms_shim.cpp (rst_io.hip and
// the output producers k_avg, k_zslice, k_extract, k_wvlcty, k_tdiag, k_uvdiag, k_particles, k_pflx)
// share: the calling thread's library state, the record description a producer
// hands the writer, the event timer of the roms_gpu_time_* entries, and the
// few calls the producers make into one another.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <utility>

#include "../../include/roms_gpu.h"
#include "k_sink.h"
#include "roms_dev.h"

namespace roms {
struct ShimState {
  Dev* d = nullptr;
  hipStream_t s = nullptr;
  const roms_dims* dims = nullptr;
  const roms_cfg* cfg = nullptr;
  std::string* err = nullptr;
};
// The entry checks of every routine (initialised, no failed halo wait, fast-
// loop exchange joined); fills S.  Returns 0 or the negative error code.
int shim_enter(ShimState& S, bool read_only = false);   // read_only: the call changes no model field
void shim_set_error(const std::string& e);
void io_free();   // rst_io.hip: joins the writer, frees staging (roms_gpu_finalize)
// A blocking copy ordered on the library's stream.  The kernels run on
// non-blocking streams, which do not wait for null-stream work, so plain
// hipMemcpy/hipMemset can race with them (a pageable hipMemcpy may return
// before its DMA has landed).
inline hipError_t copy_on(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}
void launch_fill_ones(double* p, long n, hipStream_t s);                               // k_diag.hip (self-test)
void launch_count_nonzero(const double* p, long n, unsigned long long* cnt, hipStream_t s, double v = 0.0);   // elements != v
void frc_free();  // k_forcing.hip: forcing records and tide data (roms_gpu_finalize)
// In-step forcing (roms_gpu_frc_clock, k_forcing.hip): the set_forces /
// set_bry_all / set_tides points of roms_step run inside roms_gpu_step.
// frc_step_prepare forms the step's interpolation weights on the host and
// queues them to the device before the step's kernels (0 or negative error);
// frc_step_phase enqueues the interpolations of one point (0: surface at
// 'current', 1: boundary at '1/2 fwd' + set_tides, 2: surface at '1/2 fwd',
// 3: boundary at 'forward' + set_tides), reading the weights from device
// memory so a captured step graph replays them; frc_step_gen changes
// whenever a captured graph would hold stale buffers or field lists.
int frc_step_prepare(hipStream_t s, const Dev& d, double dt, const roms_tlev& t, std::string& err);
void frc_step_phase(const Dev& d, hipStream_t s, int phase, bool pot_tides);
long frc_step_gen();
double* shim_field(int field_id);          // device array of a field (nullptr if absent)
long shim_field_dev_count(int field_id);   // elements of a field in the device layout (row pitch nx2)
// host-layout field data (the ABI's, rows of Lm+4) into a device-layout
// array of the field's shape, blocking on the library stream
hipError_t shim_field_h2d(int field_id, double* dev, const double* host);
hipError_t shim_rows_h2d(double* dev, const double* host, long rows);   // `rows` rows of Lm+4 (whole planes of Mm+4) -> device planes
// row r = p*prow + q: dst[p*dplane + q*dpitch + c] = src[p*splane + q*spitch + c], c < width (device arrays; k_diag.hip)
void launch_rows_copy(double* dst, long dpitch, long dplane, const double* src, long spitch, long splane, long width,
                      long rows, long prow, hipStream_t s);
hipError_t shim_rows_d2h(double* host, const double* dev, long rows);   // the way back: device planes -> `rows` rows of Lm+4
// ---- what a producer of output hands the record writer (rst_io.hip) ----
// one (i0:i1, j0:j1, 1:nk) block of a device field, packed i fastest
struct Slab {
  const double* src;   // element (i0, j0, level 1)
  int ni, nj, nk;
  long sj, sk;         // row and level strides
  int as_mask;         // riv_umask/riv_vmask: 1 where the river face array is non-zero
  // history omega (basic_output.F:374-384): pm*pn*(We+Wi) in m/s when src2
  // (Wi) is set; pm/pn are 2-D, element (i0, j0).  Averages omega
  // (basic_output.F:482): src is w_avg, src2 unset, (w_avg*pm)*pn in that order
  const double* src2;
  const double *pm, *pn;
};
struct OutVar {
  std::string name, lname, units;
  char grid;      // 'r', 'u', 'v'
  int levels;     // 0: 2-D; N or N+1
  int depth = 0;  // slices: planes on the depth dimension (levels 0)
  Slab slab;
  long off = 0;   // offset in the staging buffer (elements)
};
// the variable over this rank's write range (dimensions.F:40-45) of the device array `base` (element IJ = 0 of
// its first plane; planes level_stride apart)
OutVar out_var(const ShimState& S, const std::string& name, const std::string& long_name, const std::string& units,
               char grid, int levels, int depth, const double* base, long level_stride);
struct RecordSpec {
  const char* who = "roms_gpu_wrt";                          // prefix of error messages
  std::string type;                                          // the global 'type' attribute
  std::vector<std::pair<std::string, std::string>> gatts;    // text attributes after 'type'
  std::vector<OutVar> vars;
  std::vector<double> depths;                                // non-empty: a 'depth' dimension and variable (slices)
  double time = 0.0;                                         // ocean_time
};
// Record rec of the file the spec describes: packs the variables on the library stream, then drains and writes
// them on the writer thread while the model steps on.  0 once the job is queued; the caller then resets its window
int write_record(const ShimState& S, const char* path, int rec, int total_rec, const roms_tlev* t, RecordSpec spec);
// name, units and long name of every tracer (tracers.F:296-301, roms_gpu_io_tracer_name)
void io_tracer_meta(const ShimState& S, std::vector<std::string>& nm, std::vector<std::string>& un,
                    std::vector<std::string>& ln);
// a length of time as the reference writes it into a text attribute: F12.1, left-adjusted, ' seconds'
// (basic_output.F:451-455, 705; diagnostics.F:754-755)
inline std::string seconds_att(double period) {
  char tb[64];
  snprintf(tb, sizeof tb, "%.1f seconds", period);
  return tb;
}
// n rounds of `round` (a callable that enqueues one round on s and returns 0 or a negative code) between two
// events; warm: one untimed round first.  Returns the elapsed milliseconds, or the negative code
template <class F>
double time_rounds(hipStream_t s, int n, bool warm, F&& round) {
  hipEvent_t e[2];
  if (hipEventCreate(&e[0]) != hipSuccess || hipEventCreate(&e[1]) != hipSuccess) return -2.0;
  int r = 0;
  for (int q = warm ? -1 : 0; q < n && !r; q++) {
    if (q == 0) (void)hipEventRecord(e[0], s);
    r = round();
  }
  (void)hipEventRecord(e[1], s);
  float f = 0.f;
  if (hipEventSynchronize(e[1]) != hipSuccess || hipEventElapsedTime(&f, e[0], e[1]) != hipSuccess) r = r ? r : -2;
  if (!r && hipGetLastError() != hipSuccess) r = -3;
  (void)hipEventDestroy(e[0]);
  (void)hipEventDestroy(e[1]);
  return r ? (double)r : (double)f;
}
// Time-averaged output (k_avg.hip): the running means roms_gpu_calc_avg
// maintains, each in the device layout of one slot of the field it mirrors
// (nullptr: not selected), for the averages record of rst_io.hip.
struct AvgView {
  int mask = 0;        // ROMS_WRT_* bits armed (0: averaging off)
  double *zeta = nullptr, *ubar = nullptr, *vbar = nullptr, *u = nullptr, *v = nullptr, *rho = nullptr, *w = nullptr,
         *akv = nullptr, *akt = nullptr, *aks = nullptr, *hbls = nullptr, *hbbl = nullptr;
  double* wvl = nullptr;    // true vertical velocity (ROMS_WRT_W), N levels in u's layout; sampled by k_wvlcty's mean sink
  std::vector<double*> t;   // one per tracer
};
const AvgView& avg_view();
const MeanWindow& avg_window(double* t_avg);   // the open window; *t_avg: the mean time of its samples
void avg_window_written();   // wrt_avg: the next sample starts a fresh window
void avg_free();             // roms_gpu_finalize
// True vertical velocity (k_wvlcty.hip): one launch over wvlcty_tile's range from FlxU, FlxV, u, v(nstp) into `out`
// (element IJ = 0 of level 1, N planes) through the sink `sink` (k_sink.h)
int wvl_launch(const ShimState& S, int nstp, double* out, int sink, double coef, double cm1);
// N zeroed planes in the layout and alignment of one slot of u; *base is the allocation to free
double* wvl_alloc_like_u(const Dev& d, hipStream_t s, double** base);
// w of the current state into the library's work array (allocated on first use); nullptr and *rc < 0 on error
const double* wvl_compute(const ShimState& S, int nstp, int* rc);
void wvl_free();             // roms_gpu_finalize, roms_gpu_avg_begin(0)
// Tracer budget terms (k_tdiag.hip).  tdiag_record: the armed tracers' variables of a diagnostics record appended
// to `vars` (false: none is armed); *do_avg, *have: whether they are means, whether there is a sample to write
bool tdiag_record(const ShimState& S, std::vector<OutVar>& vars, bool* do_avg, bool* have);
void tdiag_window_written();   // a record took the window
void tdiag_free();             // roms_gpu_finalize
void uvdiag_free();            // roms_gpu_finalize
// Baroclinic pressure fluxes (k_pflx.hip): the filter states of the restart file and up, vp of the extraction, each in
// the device layout of one slot of u (up, vp: one plane); nullptr while not armed
struct PflxView {
  bool armed = false;
  double *u_slow = nullptr, *v_slow = nullptr, *p_slow = nullptr, *up = nullptr, *vp = nullptr;
};
PflxView pflx_view();
void pflx_free();              // roms_gpu_finalize
void zslice_free();            // roms_gpu_finalize
// Akt(isalt) made current on the library stream before a kernel or copy reads it (whole steps may leave it
// unformed while it is Akt(itemp) bit for bit: roms_shim.cpp akt_stale)
hipError_t shim_akt_sync();
bool shim_vgrid_valid();       // the stored Hz, z_r, z_w are set_depth's own (VGrid may stand in for them)
// Child-boundary extraction (k_extract.hip): one record of an extraction file
// for rst_io.hip's writer thread (its time variables and np%03d dimensions do not fit OutVar).  Every variable lies packed, (levels, np)
// point-fastest, in one device buffer that the library stream has filled.
struct ExtFileVar {
  std::string name;
  int dim_np = -1;       // index into ExtRecord::dims of its point dimension
  bool levels = false;   // on (time, s_rho, np) instead of (time, np)
  int start = 0, count = 0, dsize = 0;   // the object's start_idx, np and global length
  std::string dname, lname, units;
  long off = 0, n = 0;   // its elements in the packed buffer
};
struct ExtRecord {
  std::string time_dim;                             // the record dimension
  std::vector<std::string> time_vars;               // <set>_time of every set, in first-appearance order
  std::vector<std::pair<std::string, int>> dims;    // np%03d of every object present
  int s_rho = 0;                                    // N_chd (0: no 3-D variable)
  std::vector<ExtFileVar> vars;
  const double* dev = nullptr;
  size_t n = 0;
};
int extract_write(const char* path, int rec, double time, const ExtRecord& R);
int io_writer_join(std::string& err);   // joins the writer thread (0 or its error)
// Lagrangian particles (k_particles.hip): one record of the _part file for rst_io.hip's writer thread (its npart
// and seven dimensions do not fit OutVar).  dev: particles(npart, seven) packed on the library stream
int part_write(const ShimState& S, const char* path, int rec, double time, const double* dev, long npmx, int big_number);
void part_free();                       // roms_gpu_finalize
void extract_free();                    // roms_gpu_finalize
void shim_extract_huv(bool on);         // whole steps store Hz_u/Hz_v while an armed object reads them
bool shim_hzuv_valid();                 // the stored Hz_u/Hz_v are set_HUV's of the last step
double* shim_scratch_small(long n);      // small device scratch owned by the context (>= n doubles)
// step3d_uv2's closed-edge column lists (k_step3d_uv.hip): (dir, i, j) triples
void uv2_edge_lists(const Bounds& b, std::vector<int>& couple, std::vector<int>& flux);
}  // namespace roms
