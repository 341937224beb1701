// shim_state.h -- what the C-ABI modules outside roms_shim.cpp (rst_io.hip)
// see of the calling thread's library state.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/roms_gpu.h"
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
void io_free();
// A blocking copy ordered on the library's stream.  The kernels run on
// non-blocking streams, which do not wait for null-stream work, so plain
// hipMemcpy/hipMemset can race with them (a pageable hipMemcpy may return
// before its DMA has landed).
inline hipError_t copy_on(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}   // rst_io.hip: joins the writer, frees staging (roms_gpu_finalize)
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
// Time-averaged output (k_avg.hip): the running means roms_gpu_calc_avg
// maintains, each in the device layout of one slot of the field it mirrors
// (nullptr: not selected), for rst_io.hip's averages-file writer.
struct AvgView {
  int mask = 0;        // ROMS_WRT_* bits armed (0: averaging off)
  int navg = 0;        // samples in the open window
  double t_avg = 0.0;  // their mean time
  double *zeta = nullptr, *ubar = nullptr, *vbar = nullptr, *u = nullptr, *v = nullptr, *rho = nullptr, *w = nullptr,
         *akv = nullptr, *akt = nullptr, *aks = nullptr, *hbls = nullptr, *hbbl = nullptr;
  double* wvl = nullptr;    // true vertical velocity (ROMS_WRT_W), N levels in u's layout; sampled by k_wvlcty's mean sink
  std::vector<double*> t;   // one per tracer
};
const AvgView& avg_view();
void avg_window_written();   // wrt_avg: navg = 0, the next sample starts a fresh window
void avg_free();             // roms_gpu_finalize
// True vertical velocity (k_wvlcty.hip): one kernel body, three sinks
enum WvlSink : int { kWvlStore = 0, kWvlMean = 1, kWvlMeanFirst = 2 };   // work array | avg*cm1 + w*coef | w*coef, no load
// one launch over wvlcty_tile's range from FlxU, FlxV, u, v(nstp) into `out` (element IJ = 0 of level 1, N planes)
int wvl_launch(const ShimState& S, int nstp, double* out, int sink, double coef, double cm1);
// N zeroed planes in the layout and alignment of one slot of u; *base is the allocation to free
double* wvl_alloc_like_u(const Dev& d, hipStream_t s, double** base);
// w of the current state into the library's work array (allocated on first use); nullptr and *rc < 0 on error
const double* wvl_compute(const ShimState& S, int nstp, int* rc);
void wvl_free();             // roms_gpu_finalize, roms_gpu_avg_begin(0)
// Tracer budget terms (k_tdiag.hip): per armed tracer the six terms' device arrays (the means when do_avg), N planes
// each in a rho field's layout, [ROMS_TDIA_* - 1], for rst_io.hip's writer
struct TdiaView {
  std::vector<int> trc;                  // tracer index (1..NT) of each armed tracer
  bool do_avg = false;
  int navg = 0;                          // samples in the open window (do_avg)
  bool have = false;                     // there is a sample to write
  std::vector<const double*> term[6];    // one per armed tracer
};
const TdiaView& tdiag_view();
void tdiag_window_written();   // wrt_tdiag with do_avg: navg = 0
void tdiag_free();             // roms_gpu_finalize
// rst_io.hip: record rec of a diagnostics file (create_diagnostics_file, wrt_diag_trc) through the writer thread
int tdiag_write(const char* path, int rec, int total_rec, double time, double period, const roms_tlev* t,
                const TdiaView& tv);
// Momentum budget terms (k_uvdiag.hip): the seven terms' device arrays of u and of v (the means when do_avg), N
// planes each in the layout of u (of v), [comp][ROMS_UVD_* - 1], for rst_io.hip's writer
struct UvdView {
  bool armed = false, do_avg = false;
  int navg = 0;                          // samples in the open window (do_avg)
  bool have = false;                     // there is a complete sample to write
  const double* term[2][7] = {};
};
const UvdView& uvdiag_view();
void uvdiag_window_written();   // wrt_diag with do_avg: navg = 0
void uvdiag_free();             // roms_gpu_finalize
// rst_io.hip: record rec of a diagnostics file with the momentum terms and, tv given, the armed tracers' terms
// (create_diagvars, wrt_diag_uv, wrt_diag_trc) through the writer thread
int diag_write(const char* path, int rec, int total_rec, double time, double period, const roms_tlev* t,
               const UvdView& uv, const TdiaView* tv);
// Z-level slices (k_zslice.hip): ndep planes per sliced field in the 2-D
// device layout, zero outside cells 1..Lm x 1..Mm, for rst_io.hip's writer.
struct ZslView {
  int what = 0;        // ROMS_ZSL_* bits armed (0: slicing off)
  int ndep = 0;
  bool do_avg = false;
  int navg = 0;        // samples in the open window (do_avg)
  std::vector<double> vecdep;
  std::vector<int> trc;                // tracer index (1..NT) of each sliced tracer
  std::vector<double*> t, t_avg;       // one per sliced tracer
  double *u = nullptr, *v = nullptr, *u_avg = nullptr, *v_avg = nullptr;
};
// rst_io.hip: record rec of a slices file from the view's planes (the means
// when do_avg), through the snapshot and writer thread of the other records
int zslice_write(const char* path, int rec, int total_rec, double time, const roms_tlev* t, const ZslView& zv);
void zslice_free();            // roms_gpu_finalize
// Akt(isalt) made current on the library stream before a kernel or copy reads it (whole steps may leave it
// unformed while it is Akt(itemp) bit for bit: roms_shim.cpp akt_stale)
hipError_t shim_akt_sync();
bool shim_vgrid_valid();       // the stored Hz, z_r, z_w are set_depth's own (VGrid may stand in for them)
// Child-boundary extraction (k_extract.hip): one record of an extraction file
// for rst_io.hip's writer thread.  Every variable lies packed, (levels, np)
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
void extract_free();                    // roms_gpu_finalize
void shim_extract_huv(bool on);         // whole steps store Hz_u/Hz_v while an armed object reads them
bool shim_hzuv_valid();                 // the stored Hz_u/Hz_v are set_HUV's of the last step
double* shim_scratch_small(long n);      // small device scratch owned by the context (>= n doubles)
// step3d_uv2's closed-edge column lists (k_step3d_uv.hip): (dir, i, j) triples
void uv2_edge_lists(const Bounds& b, std::vector<int>& couple, std::vector<int>& flux);
}  // namespace roms
