// device_mat.hpp -- the library-private descriptor behind a device `spmat` handle.
//
// HBM layout (see DESIGN.md "Data layout in HBM"):
//   AS   fp64 values
//   JA   32-bit column ids (host keeps 64-bit `ulong`; narrowed during upload)
//   IRP  32-bit row pointers when NZ < 2^32, else 64-bit
//   RL   32-bit row lengths (optional)
//   ELL  row-major  [rows ][pitch(slots)]  pitch = slots rounded up to 16 elements
//        col-major  [slots][pitch(rows )]  pitch = rows  rounded up to 64 elements
//   blkInfo / blkBase  row blocks of the LDS-stream kernel (CSR only)
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "spmvHip.h"

namespace spmvhip {

constexpr int      WAVE            = 64;
constexpr int      WG_THREADS      = 256;               // 4 wavefronts
constexpr int      STREAM_NNZ      = 2048;              // nnz staged in LDS per workgroup (16 KiB of fp64)
// 32-bit row pointers are used only below this nnz count, so that `j + stride`
// in the kernels can never wrap around 2^32
constexpr uint64_t IRP32_LIMIT     = (1ull << 32) - 65536;

enum class Kind : int { CSR = 0, ELL_ROWMAJOR = 1, ELL_COLMAJOR = 2 };
// How a handle came to be (DevMat::origin; UPLOADED is also what ownCsr makes).  TRANSPOSE and later come from other handles,
// whose ids -- never pointers: a source may be freed first -- DevMat::src records: TRANSPOSE, PERMUTATION, HIERARCHY the
// source (the level-0 matrix) in src[0], PRODUCT and SUM A and B in that order, FILTER the source in src[0].  What made a
// handle refreshes it, from those handles only (madeBy in lib.hpp).  ELL_OF_CSR (spmvHipCsrToEll) keeps no link to its source, and its values cannot be updated.
// ASSEMBLED (spmvHipCooAssemble) comes from the caller's triplet arrays, not from a handle: it has no source ids.
// FSAI (spmvHipFsaiSetup) records the matrix in src[0]; the pattern handle need not outlive the setup and is not recorded.
enum class Origin : int { UPLOADED, ADOPTED, ELL_OF_CSR, TRANSPOSE, PERMUTATION, PRODUCT, HIERARCHY, SUM, FILTER, ASSEMBLED, FSAI };

struct TileFormat;          // column-sliced two-phase format, tiles.hip
struct SellFormat;          // SELL-C-sigma, sell.hip
struct StripeFormat;        // bin-wise CSC (y bins in LDS, x from the XCD's L2), stripes.hip
struct SpgemmPlan;          // what a product C = A B keeps for its refresh, spgemm.hip
struct AddPlan;             // what a sum C = alpha A + beta B keeps for its refresh, add.hip
struct FilterPlan;          // what a filtered handle keeps for its refresh besides the map, filter.hip
struct CooPlan;             // what a handle assembled from triplets keeps for its refresh, coo.hip
struct AmgHierarchy;        // the levels of an aggregation multigrid preconditioner, amg.hip
struct FsaiPlan;            // what an approximate-inverse factor G owns besides its arrays (below; fsai.hip builds the arrays)
struct TempBuf;             // a scoped device buffer, device_prims.hpp
struct TriSweepPlan;        // what the triangular solves by Jacobi sweeps keep on a handle (below; trisweep.hip builds it)

// the level sets of one triangle (built by triAnalyse in trsv.hip; the ILU(0) factorisation of ilu0.hip runs on the lower one)
struct TriSchedule {
    spmvTriInfo info{};
    uint32_t* perm = nullptr;        // rows by (level, class, id)
    uint32_t* diagPos = nullptr;     // CSR position of row i's diagonal (meaningful where the row has exactly one)
    uint32_t* levelPtr = nullptr;    // device copy of the level table (the run kernels read it)
    struct Step { uint32_t l0, l1; };           // l1 - l0 > 1: a run (one workgroup), else one level
    std::vector<uint32_t> levelPtr_h, split_h;  // level l: short rows perm[levelPtr[l], split[l]), long [split[l], levelPtr[l+1])
    std::vector<Step> steps;
};

// process-unique identity of a descriptor (never 0, never reused: a new handle at a freed one's address gets another id)
inline uint64_t newDevMatId() {
    static std::atomic<uint64_t> last{0};
    return ++last;
}

struct DevMat {
    uint32_t magic = 0x53504D56;    // 'SPMV'
    uint64_t id = newDevMatId();
    Kind     kind  = Kind::CSR;
    uint64_t M = 0, N = 0, NZ = 0;  // logical rows, cols, true nnz
    uint64_t K = 0;                 // ELL slots per row (max row nnz)
    int      irpBytes = 4;
    void*     IRP = nullptr;
    uint32_t* JA  = nullptr;
    double*   AS  = nullptr;
    uint32_t* RL  = nullptr;
    size_t    pitch = 0;            // ELL pitch in elements (same for JA and AS)
    bool      owns = true;          // false for adopted arrays
    Origin    origin = Origin::UPLOADED;
    uint64_t  src[2] = {0, 0};      // ids of the handles this one was made from (0: none)
    uint64_t  ellFirstRow = ~0ull;  // ELL with row lengths: first row that holds an entry (unit detection after a value update)
    // every stored value is the same double (MatrixMarket `pattern` files are loaded as all 1.0 -- the graphs of the
    // reference's report, asia_osm and channel-500x100x100, are such files): found at upload; the CSR kernels then take
    // the value from a register instead of streaming 8 B per entry.  c * x[j] rounds exactly as AS[j] * x[j] does.
    bool      unit = false;
    double    unitValue = 0.0;
    uint64_t  maxRowNnz = 0;
    // row blocks of the LDS-stream kernel (CSR): consecutive rows packed while their nnz <= STREAM_NNZ; a longer row is a
    // block of its own; long rows first, then row order
    uint4*    blkInfo = nullptr;    // {first row, #rows, #nnz, long-row flag}
    uint64_t* blkBase = nullptr;    // nnz offset of the block
    uint32_t  nBlk2 = 0, nLong2 = 0;
    // The two-phase format exists in two FORMS -- arrival-order and deterministic (serial-order) sums -- and the stripes
    // format in two LAYOUTS -- one stream per bin, and owner-wavefront sub-streams.  A handle may hold both of each, every
    // one in a slot of its own: tiles[deterministic], stripes[stripesLayout(mode)].  The functions of tiles.hip / stripes.hip
    // are handed the format they work on; nothing here is "the current one".  `*Pref` is the form the explicit launchers
    // and queries use: set by spmvHipBuildTilesOpt / ...StripesOpt.
    TileFormat*   tiles[2]   = {nullptr, nullptr};   // built lazily by hipSpMVTilesCSR / spmvHipBuildTiles / the selections
    StripeFormat* stripes[2] = {nullptr, nullptr};   // built lazily by hipSpMVStripesCSR / spmvHipBuildStripes / the selections
    bool      tilesPref = false;
    int       stripesPref = 0;      // 0 arrival order, 1 owner wavefronts, 2 ordered tickets (spmvStripesOpts.deterministic)
    SellFormat* sell = nullptr;     // built lazily by hipSpMVRowsSELL / spmvHipBuildSell
    // the selections: [0] among the reduction-order kernels (hipSpMVAutoCSR, hipSpMVWarpPerRowCSR), [1] among the
    // serial-order kernels (hipSpMVRowsCSR): index of the launcher chosen for this matrix (-1: not chosen yet) ...
    int       autoPick[2] = {-1, -1};
    float     autoMs[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};    // ... and what each candidate took (0 = not tried)
    spmvUpdateInfo lastUpdate{};    // what the last spmvHipUpdateValues / spmvHipValuesChanged did
    // a transpose (spmvHipCsrTranspose, transpose.hip), a permutation (spmvHipCsrPermute, colour.hip) or a filtered handle
    // (spmvHipCsrFilter, filter.hip): for every entry p of this handle, the CSR position of the same entry in the source
    // (ASt[p] = AS[tmap[p]])
    uint32_t* tmap = nullptr;
    // a product (spmvHipSpGEMM, spgemm.hip): its rows by class (4 B per row)
    SpgemmPlan* prod = nullptr;
    // a sum (spmvHipCsrAdd, add.hip): its rows by class (4 B per row)
    AddPlan* sum = nullptr;
    // a filtered handle (spmvHipCsrFilter, filter.hip): its options and, with `lump`, the keep mask and the diagonal places
    FilterPlan* filt = nullptr;
    // a handle assembled from triplets (spmvHipCooAssemble, coo.hip): its mode and, with keepMap, the sorted order of the
    // kept entries and the run starts
    CooPlan* coo = nullptr;
    // a multigrid hierarchy (spmvHipAmgSetup, amg.hip): the handle is then no matrix (no arrays, NZ = 0) and only the
    // spmvHipAmg* calls, a Krylov solve's dM and hipFreeSpmat take it
    AmgHierarchy* amg = nullptr;
    // an approximate-inverse factor (spmvHipFsaiSetup, fsai.hip): its transpose, the workspace of an apply, what the setup did
    FsaiPlan* fsai = nullptr;
    // the level-set schedules of the triangular solve (trsv.hip), [SPMV_TRI_LOWER] and [SPMV_TRI_UPPER]: built from the
    // pattern at the first solve or by spmvHipTriAnalyse, kept across value updates (the solve reads AS live)
    TriSchedule* tri[2] = {nullptr, nullptr};
    // the plan of the triangular solves by Jacobi sweeps (trisweep.hip): built by spmvHipTriSweepsPrepare, spmvHipTriSetApply
    // or the first sweep solve, kept across value updates (the sweeps read AS live), never with level sets
    TriSweepPlan* sweep = nullptr;
    // the ILU(0) factorisation (ilu0.hip): what its pattern check found (checked once, kept across value updates) and
    // what the last call did
    bool      iluChecked = false;
    long      iluUnsortedRow = -1;  // the first row whose columns are not strictly ascending
    // AS holds the complete factors of a hipSpILU0CSR whose last step (the unit flag, the built formats) failed: the same
    // call made again finishes the handle and must not factorise the factors.  Whatever writes AS clears it before it
    // writes: spmvHipUpdateValues / ValuesChanged (updateValues) and the refreshes of a derived handle (upload.hip).
    bool      iluPending = false;
    spmvIluInfo ilu{-1, -1, 0, 0, 0, 0, 0.0};
    // the single-precision form of the values (spmvHipValuesF32, values_f32.hip): AS32[p] = (float)AS[p] for the NZ entries,
    // with the 32 bytes of the demotion's counters behind them in the same allocation; a unit handle has no array, only
    // its register value rounded the same way.  It follows AS through updateValues like the formats above.
    bool      f32 = false;          // the form is built (a unit handle: without an array)
    float*    AS32 = nullptr;
    double    unitValue32 = 0.0;    // (double)(float)unitValue
    spmvF32Info f32Info{0, 0, 0, 0, 0, 0, 0, -1};
};

// What the sweep solves keep: the diagonal's places, what the pattern pass found, two M x width iterates
// (ws, then ws + M * width), and how a Krylov solve applies this handle as dM.  The row blocks are the handle's blkInfo / blkBase.
struct TriSweepPlan {
    uint32_t* diagPos = nullptr;    // CSR position of row i's diagonal (meaningful where the row has exactly one)
    double*   ws = nullptr;
    uint32_t  width = 0;            // columns the iterates hold
    long      firstBadDiag = -1;    // -1, or the first row without exactly one stored diagonal entry
    bool      sorted = false;       // every row ascends strictly and holds one diagonal entry (the ILU(0) precondition)
    int       mode = 0;             // SPMV_TRI_APPLY_EXACT | SPMV_TRI_APPLY_SWEEPS
    uint32_t  sweeps[2] = {0, 0};   // lower, upper sweeps of one application in SWEEPS mode
    int       prepares = 0;
    unsigned long solveLaunches = 0;   // kernels the last sweep solve enqueued
};

// What a factor G of spmvHipFsaiSetup owns privately: G^T (made and refreshed by the transpose path, with a handle of its own
// for the launchers), a handle over G itself for them, one M-vector for G r, the forced group width and the last report.
struct FsaiPlan {
    int      storage = 0;           // SPMV_STORAGE_F64 | SPMV_STORAGE_F32 (spmvHipFsaiSetStorage): which products an apply takes
    DevMat*  gt = nullptr;
    spmat    hG{}, hGT{};
    double*  work = nullptr;
    uint32_t lanes = 0;             // spmvFsaiOpts.lanesPerRow (0: the built-in choice)
    spmvFsaiInfo info{0, 0, 0, -1, 0, 0, 0.0};
};

// The one place that looks at the width of the row pointers: f (a generic lambda) is called with them as const uint32_t*
// or const uint64_t*; IrpT<decltype(irp)> names the integer for a kernel's template argument.
template <typename P> using IrpT = std::remove_const_t<std::remove_pointer_t<P>>;
template <typename F>
auto withIrp(const void* IRP, int irpBytes, F&& f) {
    return irpBytes == 4 ? f(static_cast<const uint32_t*>(IRP)) : f(static_cast<const uint64_t*>(IRP));
}
template <typename F> auto withIrp(const DevMat* d, F&& f) { return withIrp(d->IRP, d->irpBytes, f); }
// ... of two handles (the sparse product and the sparse sum): f(irpA, irpB)
template <typename F> auto withBoth(const DevMat* a, const DevMat* b, F&& f) {
    return withIrp(a, [&](auto ia) { return withIrp(b, [&](auto ib) { return f(ia, ib); }); });
}

int  buildSell(DevMat* d);                                      // sell.hip
void freeSell(SellFormat* f);
int  enqueueSell(DevMat* d, const double* x, double* y, hipStream_t stream);
size_t sellBytes(const DevMat* d);

// the stripes layout of a launch mode (spmvStripesOpts.deterministic, DevMat::stripesPref): 0 arrival order and 2 ordered tickets
// share the one-stream-per-bin layout [0], 1 owner wavefronts has the sub-stream layout [1]
inline int stripesLayout(int mode) { return mode == 1; }
// Builds: nullptr = the automatic format of slot 0, kept if it exists; explicit options replace the format of the slot they name
// and leave the other alone.  Every other function is handed the format it works on (null where noted: an empty answer).
int  buildStripes(DevMat* d, const spmvStripesOpts* opts = nullptr);   // stripes.hip
void freeStripes(StripeFormat* f);
int  enqueueStripes(const StripeFormat* f, const double* x, double* y, hipStream_t stream, int mode, dim3* grid = nullptr, dim3* block = nullptr);
size_t stripesBytes(const DevMat* d);                           // both layouts
void stripesInfo(const StripeFormat* f, spmvStripesInfo* out);  // f may be null

int  buildTiles(DevMat* d, const spmvTilesOpts* opts = nullptr); // tiles.hip
void tilesInfo(const TileFormat* t, spmvTilesInfo* out);        // t may be null
void freeTiles(TileFormat* t);
void peerFinalize();                                            // peer.hip: the copy streams of the push exchange
void freeTilesWorkspace();                                      // the per-device product workspace (8 B/nnz of the largest matrix)
int  enqueueTiles(const DevMat* d, const TileFormat* t, const double* x, double* y, hipStream_t stream);
int  enqueueTilesExpand(const DevMat* d, const TileFormat* t, const double* x, hipStream_t stream);
int  enqueueTilesReduce(const DevMat* d, const TileFormat* t, uint32_t binBegin, uint32_t binEnd, double* y, int nExtra, double* const* extra,
                        hipStream_t stream);
int  enqueueTilesReducePush(const DevMat* d, TileFormat* t, double* y, int nExtra, double* const* extra, hipStream_t stream, hipStream_t side,
                            hipEvent_t evFork, hipEvent_t evJoin);
int  tilesPushFailed(const TileFormat* t);                      // t may be null
void tilesShape(const TileFormat* t, uint32_t* bins, uint32_t* rowsPerBin);   // t may be null
uint32_t tilesPhase2Threads(const TileFormat* t);               // workgroup size of phase 2
uint64_t tilesBinRow(const DevMat* d, const TileFormat* t, uint32_t bin);
hipStream_t libraryStream();                                    // abi.hip: the stream set with spmvHipSetStream
size_t tilesBytes(const DevMat* d);                             // both forms

// Value refresh (values.hip and the format files).  Each format rewrites its value array from the handle's CSR `AS`
// (already updated) on `stream`; the map from storage to CSR order is built at a format's first refresh (*mapMs grows by
// its build time).  Index arrays, tables and addresses stay as they are.
int  tilesRefreshValues(DevMat* d, TileFormat* t, hipStream_t stream, double* mapMs, int* mapsBuilt);       // tiles.hip
int  stripesRefreshValues(DevMat* d, StripeFormat* f, hipStream_t stream, double* mapMs, int* mapsBuilt);   // stripes.hip
bool stripesHasValues(const StripeFormat* f);                  // false: built for a unit matrix, no value array to refresh
spmvStripesOpts stripesOptions(const StripeFormat* f);          // what the format was built with
void stripesSetUnit(StripeFormat* f, bool unit, double value);
int  sellRefreshValues(DevMat* d, hipStream_t stream);          // sell.hip
// A^T of a CSR handle on `stream` (transpose.hip): t->IRP (4 B), t->JA, t->AS and t->tmap are allocated by the caller
// for a->N + 1 rows / a->NZ entries; the temporaries are freed before the call returns, and it returns with the stream
// synchronised
int  transposeCsr(const DevMat* a, DevMat* t, hipStream_t stream);
// the pieces of the transpose that the triangular analysis and the colouring share (transpose.hip): ptr[c] = the first of
// the nnz sorted keys that is >= c, for c in [0, N] (keys >= N clamp to N); rowOf[p] = the row of CSR position p; and the
// pattern sorted by column: the stable sort of (keys, payload) over `bits` key bits into (keysOut, payloadOut), its
// workspace in ws (which must outlive what is enqueued), then ptr from keysOut -- the bounds also when nnz is 0
void enqueueSortedBounds(uint64_t nnz, uint64_t N, const uint32_t* keys, uint32_t* ptr, hipStream_t stream);
void enqueueRowOf(uint64_t M, const void* IRP, int irpBytes, uint32_t* rowOf, hipStream_t stream);
hipError_t enqueueSortedByColumn(uint64_t nnz, uint64_t N, unsigned bits, uint32_t* keys, uint32_t* payload, uint32_t* keysOut,
                                 uint32_t* payloadOut, uint32_t* ptr, TempBuf& ws, hipStream_t stream);
// Multi-colour ordering and symmetric permutation (colour.hip; contracts in spmvHip.h, design in DESIGN.md section 21).
// colourCsr: the colours and the (colour, id) order of the checked square handle, K rounds per host check; dColour / dPerm
// may be null; synchronous, allocates, temporaries freed before it returns.  invertPerm: inv = perm^-1 into the caller's M
// words, *bad != 0 when perm is no permutation of 0..M-1 (synchronous).  permuteCsr: B = P A P^T into t, whose IRP (4 B), JA,
// AS and tmap the caller has allocated for M + 1 rows / NZ entries, as transposeCsr.  enqueueVecPermute: kernels only.
int  colourCsr(const DevMat* a, int order, uint32_t seed, uint32_t K, uint32_t* dColour, uint32_t* dPerm, spmvColourInfo* info,
               hipStream_t stream);
int  invertPerm(uint64_t M, const uint32_t* perm, uint32_t* inv, uint32_t* bad, hipStream_t stream);
int  permuteCsr(const DevMat* a, const uint32_t* inv, DevMat* t, hipStream_t stream);
int  enqueueVecPermute(uint64_t n, const uint32_t* perm, const double* in, double* out, int inverse, hipStream_t stream);
// Reverse Cuthill-McKee ordering (rcm.hip; contract in spmvHip.h, design in DESIGN.md section 37) of the checked square handle:
// peripheral != 0 searches a pseudo-peripheral start in at most maxPasses (>= 1) passes, forward != 0 leaves the order
// unreversed, T (at most 1024; 0: never) is the frontier up to which the single-workgroup run expands a level itself.  dPerm
// may be null, info not; synchronous, allocates, temporaries freed before it returns; info is written on success only.
int  rcmCsr(const DevMat* a, int peripheral, uint32_t maxPasses, int forward, uint32_t T, uint32_t* dPerm, spmvRcmInfo* info,
            hipStream_t stream);
// C = A B (spgemm.hip; contract in spmvHip.h, design in DESIGN.md section 22).  spgemmBuild: c has kind, M and N set and owns
// nothing; on success it owns IRP (4 B), JA, AS and the plan, with NZ set; on failure the caller frees c with whatever it
// holds.  spgemmRefresh: the numeric phase again into c's arrays.  Both synchronous, temporaries freed before they return.
int  spgemmBuild(const DevMat* a, const DevMat* b, const spmvSpgemmOpts* opts, DevMat* c, spmvSpgemmInfo* info, hipStream_t stream);
int  spgemmRefresh(DevMat* c, const DevMat* a, const DevMat* b, spmvSpgemmInfo* info, hipStream_t stream);
void freeSpgemmPlan(SpgemmPlan* p);
// C = alpha A + beta B (add.hip; contract in spmvHip.h, design in DESIGN.md section 25), as the product: addBuild fills c (kind,
// M and N set, nothing owned) with IRP (4 B), JA, AS and the plan, NZ set -- on failure the caller frees c with whatever it
// holds --, addRefresh runs the numeric phase again into c's arrays.  Both synchronous, temporaries freed before they return.
int  addBuild(double alpha, const DevMat* a, double beta, const DevMat* b, const spmvAddOpts* opts, DevMat* c, spmvAddInfo* info,
              hipStream_t stream);
int  addRefresh(DevMat* c, double alpha, const DevMat* a, double beta, const DevMat* b, spmvAddInfo* info, hipStream_t stream);
void freeAddPlan(AddPlan* p);
// C = the entries of A that a predicate keeps (filter.hip; contract in spmvHip.h, design in DESIGN.md section 29).  filterBuild
// fills c (kind, M and N set, nothing owned) with IRP (4 B), JA, AS, the map to A's positions and the plan, NZ set, for
// checked options -- on failure the caller frees c with whatever it holds.  filterRefresh: after A's current values were
// gathered through the map, the ordered sums of `lump` again over the build's dropped places.  Both synchronous, temporaries
// freed before they return.  filterInfo: what the build or the last refresh did; filterSetMaxRow takes the longest row
// from the finished handle.
int  filterBuild(const DevMat* a, const spmvFilterOpts* opts, DevMat* c, hipStream_t stream);
int  filterRefresh(DevMat* c, const DevMat* a, hipStream_t stream);
const spmvFilterInfo* filterInfo(const DevMat* c);
void filterSetMaxRow(DevMat* c);
void freeFilterPlan(FilterPlan* p);
// C from COO triplets (coo.hip; contract in spmvHip.h, design in DESIGN.md section 36).  cooBuild fills c (kind, M and N set,
// nothing owned) with IRP (4 B), JA, AS and the plan, NZ set, from checked arguments -- on failure it has written its line and
// the caller frees c with whatever it holds.  cooRefresh: the values again from a new value list over the build's runs, kernels
// only.  csrToCoo: a CSR handle's entries as triplets into the caller's arrays, kernels and copies only.  All synchronous.
// cooInfo: what the build or the last refresh did; cooSetMaxRow takes the longest row from the finished handle; cooHasMap /
// cooEntries: what a refresh checks.
int  cooBuild(uint64_t nEntries, const uint32_t* dRow, const uint32_t* dCol, const double* dVal, const spmvCooOpts* opts, DevMat* c,
              hipStream_t stream);
int  cooRefresh(DevMat* c, const double* dVal, hipStream_t stream);
int  csrToCoo(const DevMat* a, uint32_t* dRow, uint32_t* dCol, double* dVal, hipStream_t stream);
const spmvCooInfo* cooInfo(const DevMat* c);
void cooSetMaxRow(DevMat* c);
bool cooHasMap(const DevMat* c);
uint64_t cooEntries(const DevMat* c);
void freeCooPlan(CooPlan* p);
// The approximate-inverse factor (fsai.hip; contract in spmvHip.h, design in DESIGN.md section 38).  fsaiBuild fills g (kind,
// M and N set, nothing owned) with IRP (4 B), JA and AS for the checked handles a and s (the pattern; s may be a), NZ set --
// on failure the caller frees g with whatever it holds; *longRow >= 0 names a pattern row above SPMV_FSAI_MAX_ROW, for which
// nothing was printed.  fsaiValues: the values of g again from a's current values (lanes: a forced group width or 0, maxRow:
// the longest row of g); its one allocation comes before its first write.  Both synchronous, temporaries freed before they
// return; info's nnz, maxRow, badRows, firstBadRow are set and launches grows.  fsaiLanes: the group width a call takes.
int  fsaiBuild(const DevMat* a, const DevMat* s, DevMat* g, uint32_t lanes, spmvFsaiInfo* info, long* longRow, hipStream_t stream);
int  fsaiValues(const DevMat* a, DevMat* g, uint32_t lanes, uint32_t maxRow, spmvFsaiInfo* info, hipStream_t stream);
uint32_t fsaiLanes(uint32_t forced, uint64_t M, uint64_t nnz);
// A dense rows x k block of doubles in the form the C boundary is given, checked there (lib.hpp: denseOperand, denseShare):
// element (i, c) at p[i*ld + c] (rowMajor) or p[c*ld + i].  Every block launcher below takes its operands as this; one that
// only reads takes the same type.  A solver's own n x kp workspace block is Dense{p, kp, true}.
struct Dense {
    double* p; uint64_t ld; bool rowMajor;
    uint64_t sr() const { return rowMajor ? ld : 1; }             // elements from a row to the next, and
    uint64_t sc() const { return rowMajor ? 1 : ld; }             // from a column to the next
};
// Aggregation multigrid (aggregate.hip, amg.hip; contracts in spmvHip.h, design in DESIGN.md sections 24 and 31).
// aggregateCsr: the aggregate ids of the checked square handle into dAgg (M words), K rounds per host check; synchronous,
// allocates, temporaries freed before it returns.  AmgPlan: which of the three setups a hierarchy is, with that setup's
// checked numbers (0: the default, and what a kind does not use).  amgBuild: the hierarchy of the checked handle hA into
// m->amg (on failure the caller frees m with whatever it holds).  amgRefresh: every level's recipe again, in place.
// enqueueAmgCycle: z = V(0, r), kernels only on `stream`; every kernel of the cycle but its SpMVs returns at once when `stop`
// is set and *stop != 0; *launches grows by the kernels enqueued (an SpMV counted as one).  amgSetSmoother: the cycle's
// smoother and sweep counts from checked options (synchronous, allocates the tables; a failure leaves the hierarchy as it
// was).  amgInfo: what the setup or the last refresh did.  The views: amgLevel / amgSmoother of a level below amgInfo()->levels,
// amgProlongator / amgStrength of one below the last.  ownCsr (upload.hip): a CSR handle that owns three device arrays.
enum class AmgKind { PLAIN, SMOOTHED, STRENGTH };              // unit prolongator; P = T - w D^-1 A T; that on the filtered A
struct AmgPlan {
    AmgKind kind = AmgKind::PLAIN;
    double omegaP = 0.0, theta = 0.0, thetaScale = 0.0;     // the damping of P (0: (4/3) / rho_l); theta_0 and theta_{l+1} / theta_l
    uint32_t fuseMax = 0, K = 16;       // the longest row of P that the fused correction takes (0: never); aggregation rounds per host check
};
int  amgSetSmoother(DevMat* m, spmat* hA, const spmvAmgSmootherOpts* opts, hipStream_t stream);
void amgSmoother(const DevMat* m, unsigned level, spmvAmgSmootherInfo* info);
// amgSetGaussSeidel: the multicolour Gauss-Seidel smoother from checked options, as amgSetSmoother (a failure leaves the
// hierarchy as it was): a level of at most smallRows rows sweeps in one workgroup, a row takes `lanes` lanes (1, 4 .. 64; 0:
// by the level's mean row), the colourings take colourK rounds per host check.  amgGaussSeidel: the view of a level below amgInfo()->levels.
int  amgSetGaussSeidel(DevMat* m, spmat* hA, const spmvAmgGsOpts* opts, uint32_t smallRows, uint32_t lanes, uint32_t colourK, hipStream_t stream);
void amgGaussSeidel(const DevMat* m, unsigned level, spmvAmgGsInfo* info);
int  aggregateCsr(const DevMat* a, uint32_t seed, uint32_t K, uint32_t* dAgg, spmvAggInfo* info, hipStream_t stream);
int  amgBuild(spmat* hA, const spmvAmgOpts* opts, const AmgPlan& plan, DevMat* m, hipStream_t stream);
int  amgRefresh(DevMat* m, spmat* hA, hipStream_t stream);
int  enqueueAmgCycle(const DevMat* m, spmat* hA, const double* r, double* z, hipStream_t stream, const uint32_t* stop,
                     unsigned long* launches);
// The block cycle.  amgSetBlockWidth: the workspace of a cycle for up to `width` columns, 0 drops it
// (synchronous, allocates; a failure leaves the hierarchy as it was).  amgBlockState: the width, the workspace's bytes, and
// whether a level sweeps by colours (which the block cycle does not).  enqueueAmgCycleBlock: Z(:, c) = V(0, R(:, c)) for
// c < k <= the width on a hierarchy without a Gauss-Seidel level, a0 its source; R and Z the caller's blocks; kernels
// only, `stop` and `launches` as in enqueueAmgCycle (an SpMM pass of any width counted as one).
int  amgSetBlockWidth(DevMat* m, uint32_t width, hipStream_t stream);
void amgBlockState(const DevMat* m, uint32_t* width, uint64_t* bytes, bool* gaussSeidel);
int  enqueueAmgCycleBlock(const DevMat* m, const DevMat* a0, uint32_t k, const Dense& R, const Dense& Z, hipStream_t stream,
                          const uint32_t* stop, unsigned long* launches);
int  amgSetStorage(DevMat* m, spmat* hA, int storage, hipStream_t stream);      // section 41: the cycle's products from f32 forms
void amgStorage(const DevMat* m, spmvAmgStorageInfo* info);
const spmvAmgInfo* amgInfo(const DevMat* m);
void amgLevel(const DevMat* m, unsigned level, spmat* dAl, const uint32_t** dAgg, const double** dDinv);
void amgProlongator(const DevMat* m, unsigned level, spmat* dPl, spmat* dRl, double* omegaP);
bool amgIsStrength(const DevMat* m);
void amgStrength(const DevMat* m, unsigned level, spmat* dFl, double* theta);
void freeAmg(AmgHierarchy* h);
int  ownCsr(spmat* dst, uint64_t M, uint64_t N, uint64_t NZ, uint32_t* dIRP, uint32_t* dJA, double* dAS);
// Triangular solves (trsv.hip; contract in spmvHip.h, design in DESIGN.md section 17).  triAnalyse builds d->tri[uplo]
// (synchronous, allocates, temporaries freed before it returns; runThreshold = the T of the single-workgroup runs, 0: none);
// enqueueTrsv enqueues one solve of an analysed triangle on `stream` (no allocation, no sync) and reports the last launch;
// every launch returns at once when `stop` is set and *stop != 0 when it starts (a stopped Krylov loop, krylov.hip).
int  triAnalyse(DevMat* d, int uplo, uint32_t runThreshold, hipStream_t stream);
int  enqueueTrsv(const DevMat* d, int uplo, int diag, const double* b, double* x, hipStream_t stream, dim3* grid, dim3* block,
                 const uint32_t* stop = nullptr);
void triInfo(const DevMat* d, int uplo, spmvTriInfo* out);
void freeTri(TriSchedule* s);
// X = T^-1 B for k columns on the analysed triangle's schedule (trsm.hip; contract in spmvHip.h, design in DESIGN.md section
// 26): B is read by its strides, X's layout picks the kernel instance; as many launches as enqueueTrsv
// makes, whatever k is, on `stream`, no allocation, no sync; reports the last launch; `stop` as enqueueTrsv's (the block
// Krylov loops, krylov_block.hip).  The caller has checked the arguments.
int  enqueueTrsm(const DevMat* d, int uplo, int diag, uint32_t k, const Dense& B, const Dense& X, hipStream_t stream, dim3* grid,
                 dim3* block, const uint32_t* stop = nullptr);
// Triangular solves by Jacobi sweeps (trisweep.hip; contract in spmvHip.h, design in DESIGN.md section 40).  triSweepsPrepare
// builds d->sweep for `width` columns (0: one) or widens its iterates: synchronous, allocates, never level sets; a failure
// leaves the handle as it was.  enqueueTriSweeps: X = x(S) for k <= the width columns of a prepared handle; enqueueTriSweepsApply:
// out = U~^-1 (L~^-1 in) with the plan's counts, in and out distinct blocks.  Both: kernels only on `stream`, every one
// returns at once when `stop` is set and *stop != 0, *launches grows by the kernels enqueued.  triSweepsMode: d is applied
// by sweeps as a dM.  The two counts: what a solve and an application enqueue.
int  triSweepsPrepare(DevMat* d, uint32_t width, hipStream_t stream);
int  enqueueTriSweeps(const DevMat* d, int uplo, int diag, uint32_t sweeps, uint32_t k, const Dense& B, const Dense& X, hipStream_t stream,
                      dim3* grid, dim3* block, const uint32_t* stop, unsigned long* launches);
int  enqueueTriSweepsApply(const DevMat* d, uint32_t k, const Dense& in, const Dense& out, hipStream_t stream, const uint32_t* stop,
                           unsigned long* launches);
bool triSweepsMode(const DevMat* d);
unsigned long triSweepsSolveLaunches(uint32_t sweeps, bool dunit, bool inPlace);
unsigned long triSweepsApplyLaunches(uint32_t lower, uint32_t upper);
void freeTriSweeps(TriSweepPlan* p);
// ILU(0) in place on the lower schedule d->tri[SPMV_TRI_LOWER] (ilu0.hip; contract in spmvHip.h, design in DESIGN.md section
// 18).  iluUnsortedRow: the first row that is not strictly ascending, or -1 (synchronous).  iluFactor: the factorisation's
// launches on `stream` for the checked handle, then the zero-pivot read-back (synchronous); groupWidth 8, 16 or 64 lanes
// per row; fills d->ilu's zeroPivot, levels, launches and longRows.
int  iluUnsortedRow(const DevMat* d, hipStream_t stream, long* row);
int  iluFactor(DevMat* d, uint32_t groupWidth, hipStream_t stream);
// Krylov solves (krylov.hip; contract in spmvHip.h, design in DESIGN.md section 19).  enqueueDot: the fixed-order dot
// product into one device double on `stream`, its block partials in a library workspace grown (synchronously) when a call
// needs more; freeDotWorkspace gives it back.  krylovSolve: CG (bicg = 0) or BiCGStab on the checked handles a / hA, m the
// analysed ILU(0) handle or null, K iterations per host check; allocates its workspace, synchronous.
int  enqueueDot(uint64_t n, const double* u, const double* v, double* result, hipStream_t stream);
void freeDotWorkspace();
int  krylovSolve(int bicg, spmat* hA, const DevMat* a, const DevMat* m, const double* b, double* x, const spmvKrylovOpts* opts,
                 spmvKrylovInfo* info, uint32_t K, hipStream_t stream);
// Blocks of right-hand sides (krylov_block.hip; contract in spmvHip.h, design in DESIGN.md sections 27 and 34).
// enqueueBlockDot: k fixed-order dots U(:, c) . V(:, c) into k device doubles, partials
// in the dot workspace.  krylovBlockSolve: k solves in lock step on the checked handles, m the analysed ILU(0) handle or
// null, K iterations per read-back of the all-stopped word; allocates its workspace, synchronous.
int  enqueueBlockDot(uint64_t n, uint32_t k, const Dense& U, const Dense& V, double* out, hipStream_t stream);
int  krylovBlockSolve(int bicg, const DevMat* a, const DevMat* m, uint32_t k, const Dense& B, const Dense& X,
                      const spmvKrylovOpts* opts, spmvKrylovColumn* cols, spmvKrylovInfo* info, uint32_t K, hipStream_t stream);
// h = V^T w and restarted GMRES (gmres.hip; contract in spmvHip.h, design in DESIGN.md section 20).  enqueueMultiDot: k
// fixed-order dots in one pass into k device doubles, partials in the dot workspace (grown to k blocks-of-n).  gmresSolve:
// GMRES(restart) with CGS2 on the checked handles; fused != 0 folds the first update into the second projection's
// partials; allocates gmresWorkspaceBytes, synchronous.
int  enqueueMultiDot(uint64_t n, uint32_t k, const double* V, uint64_t ldv, const double* w, double* out, hipStream_t stream);
// Y = V S and thick-restart Lanczos (lanczos.hip; contract in spmvHip.h, design in DESIGN.md section 39).
// enqueueBlockCombine: one kernel (none for n = 0) on checked operands, *grid its shape.  lanczosSolve: the loop on the
// checked handle and options; allocates lanczosWorkspaceBytes, synchronous; theta, res, X and info are written only on
// EXIT_SUCCESS.  lanczosDefaultKeep: the columns a restart keeps when opts.keep == 0.
int  enqueueBlockCombine(uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* S, uint64_t lds, double* Y,
                         uint64_t ldy, hipStream_t stream, dim3* grid);
unsigned lanczosDefaultKeep(unsigned nev, unsigned ncv);
size_t lanczosWorkspaceBytes(uint64_t n, uint32_t ncv);
int  lanczosSolve(spmat* hA, const DevMat* a, const double* v0, const spmvLanczosOpts* opts, double* X, uint64_t ldx, double* theta,
                  double* res, spmvLanczosInfo* info, hipStream_t stream);
// R = W S - (V S) diag(theta) with its column norms, and generalised Davidson (davidson.hip; contract in spmvHip.h, design in
// DESIGN.md section 42).  enqueueBlockResidual: the pass and the finish of its k norms (nothing for n = 0) on checked
// operands, the block partials in `part` (k blocks-of-n doubles), flags null or {stop, skip} of a solve, *grid the pass's
// shape.  blockResidual: the same with the partials in the dot workspace.  davidsonSolve: the loop on the checked handles and
// options (m: the checked dM or null); allocates davidsonWorkspaceBytes, synchronous; theta, res, X and info are written only
// on EXIT_SUCCESS.
int  enqueueBlockResidual(uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* W, uint64_t ldw, const double* S,
                          uint64_t lds, const double* theta, double* R, uint64_t ldr, double* part, double* norm2, const uint32_t* flags,
                          hipStream_t stream, dim3* grid);
int  blockResidual(uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* W, uint64_t ldw, const double* S,
                   uint64_t lds, const double* theta, double* R, uint64_t ldr, double* norm2, hipStream_t stream, dim3* grid);
size_t davidsonWorkspaceBytes(uint64_t n, uint32_t ncv, uint32_t nev, int precond);
int  davidsonSolve(spmat* hA, const DevMat* a, const DevMat* m, const double* v0, const spmvDavidsonOpts* opts, double* X, uint64_t ldx,
                   double* theta, double* res, spmvDavidsonInfo* info, hipStream_t stream);
size_t gmresWorkspaceBytes(uint64_t n, uint32_t restart, uint64_t maxIter, int precond, int history);
int  gmresSolve(spmat* hA, const DevMat* a, const DevMat* m, const double* b, double* x, const spmvGmresOpts* opts,
                spmvKrylovInfo* info, int fused, hipStream_t stream);
int  enqueueGatherValues(double* val, const uint32_t* map, uint64_t n, const double* AS, hipStream_t stream);   // values.hip
int  enqueueScatterValues(double* val, const uint32_t* map, uint64_t n, const double* AS, hipStream_t stream);
int  enqueueSellValues(uint32_t nSlices, const uint64_t* sliceOff, const uint32_t* perm, const uint32_t* slen, const void* IRP,
                       int irpBytes, const double* AS, double* val, hipStream_t stream);
int  updateValues(spmat* h, const double* AS, bool onDevice, bool reread, hipStream_t stream, const char* who);   // upload.hip
// Y = A X for k columns, X of N rows and Y of M (spmm.hip): one launch per panel of at
// most 16 columns on `stream`, no allocation; the caller has checked handle, pointers and extents
int  enqueueSpmm(const DevMat* d, uint32_t k, const Dense& X, const Dense& Y, hipStream_t stream, bool f32 = false);
// The single-precision value form of a CSR handle (values_f32.hip; contract in spmvHip.h, design in DESIGN.md section 41).
// valuesF32Set: build (on) or release the form of the checked CSR handle; synchronous on `stream`; a failed build leaves no
// form.  valuesF32Follow: what updateValues calls after the unit detection when the form is built -- the new roundings at the
// same address, the array made or freed on a unit transition; a failure has written its line and left the form not built.
// valuesF32Drop: the form given back (the values it followed are gone).
int  valuesF32Set(DevMat* d, int on, hipStream_t stream, const char* who);
int  valuesF32Follow(DevMat* d, hipStream_t stream, const char* who);
void valuesF32Drop(DevMat* d);
bool liveShard(const void* p);                                  // shard.hip: p is a live handle of spmvHipShardCSR
constexpr uint32_t VMAP_NONE = 0xFFFFFFFFu;                    // map entry of a padding cell (value 0.0); nnz < 2^32 - 65536

// Fold `blocks` workgroups into an (x, y) grid whose x extent keeps
// x * threads < 2^32 (AQL grid_size is 32-bit work-items per dimension).
// Kernels use linear_block() and bounds-check against the real block count.
inline dim3 grid2d(uint64_t blocks, unsigned threads) {
    const uint64_t maxX = ((1ull << 32) - 1) / threads;         // >= 4 M blocks for <= 1024 threads
    if (blocks <= maxX) return dim3((unsigned)(blocks ? blocks : 1), 1, 1);
    const uint64_t gx = 1ull << 20;
    return dim3((unsigned)gx, (unsigned)((blocks + gx - 1) / gx), 1);
}

// Every device allocation and release of the library goes through these two (abi.hip, over alloc_ledger.hpp): the ledger
// knows what is held, and spmvHipAllocRefuse can make the n-th allocation fail.  devMalloc returns what the runtime
// returned (a refusal leaves *p null and the runtime's sticky error set, as a failed hipMalloc does); devFree(null) is
// nothing.
hipError_t devMalloc(void** p, size_t bytes);
hipError_t devFree(void* p);
template <typename T> hipError_t devMalloc(T** p, size_t bytes) { return devMalloc(reinterpret_cast<void**>(p), bytes); }

// a failed call is reported HERE, once: the runtime's sticky last-error is cleared so that the next, unrelated call's
// hipGetLastError() does not see it (a failed hipMalloc of a format build used to make the next spmvHipVecFill "fail")
inline bool hipOk(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    fprintf(stderr, "\33[31m\33[1m\33[44mlibspmvhip: %s\t%s\33[0m\n", what, hipGetErrorString(e));
    return false;
}
#define HIP_TRY(expr) do { if (!::spmvhip::hipOk((expr), #expr)) return EXIT_FAILURE; } while (0)

// One 32-bit word on the device for a kernel to flag something in: allocated, every byte set to `init`, written by what
// launch(word) enqueues on `stream`, read back into *out on that stream (synchronised) and freed.  A failure is reported
// and leaves no sticky error behind; *out is then untouched.
template <typename L>
int deviceFlag(int init, hipStream_t stream, const char* kernel, uint32_t* out, L&& launch) {
    uint32_t* dFlag = nullptr;
    HIP_TRY(devMalloc(&dFlag, 4));
    bool ok = hipOk(hipMemsetAsync(dFlag, init, 4, stream), "hipMemset");
    if (ok) launch(dFlag);
    ok = ok && hipOk(hipGetLastError(), kernel) && hipOk(hipMemcpyAsync(out, dFlag, 4, hipMemcpyDeviceToHost, stream), "hipMemcpy") &&
         hipOk(hipStreamSynchronize(stream), "hipStreamSynchronize");
    (void)devFree(dFlag);
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

}  // namespace spmvhip
