/*
 * spmvHip.h -- C-ABI of libspmvhip.so: the MI355X (gfx950) replacement for the
 * reference's CUDA path.  Plain C, plain pointers and sizes; no C++/torch types.
 *
 * Every entry point returns EXIT_SUCCESS (0) / EXIT_FAILURE (1) like the
 * reference's host functions (cudaUtils.cu:45,54; SpMV_CSR_OMP.c:35,61), prints
 * its diagnostics on stderr and NEVER calls exit() (the reference's
 * checkCudaErrors does, cudaUtils.h:26-34 -- not reproduced).
 *
 * What each group replaces in the reference (paths relative to its root):
 *   upload / free ......... src/include/cudaUtils.h:60-78, src/commons/cudaUtils.cu:20-98
 *   SpMV launchers ........ the five __global__ kernels of src/SpMV_CUDA.cu:33-135 as the
 *                           drivers invoke them: f<<<grid,block>>>(dMat,dVect,Conf,dOutV)
 *                           (src/main.cu:233, test/SpMV_test.cu:112)
 *   vectors / lifecycle ... the cudaMalloc/cudaMemcpy/cudaFree calls the drivers make inline
 *                           (src/main.cu:195-199,245-247,277-280)
 *   sharding .............. new (the reference is single-GPU); see DESIGN.md "Multi-GPU"
 */
#ifndef SPMV_HIP_H
#define SPMV_HIP_H

#include "spmv_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ lifecycle */
/* Select device `dev` for the calling thread and check the caller was compiled
 * against the same struct layouts.  Must be called once before anything else. */
int spmvHipInit(int dev, size_t sizeofSpmat, size_t sizeofConfig);
/* Gives back everything the library holds on its own account: the cached device copies of the host-pointer wrappers, the
 * per-device product workspace of the two-phase kernel, its side streams and events.  Handles made by spMatCpy* stay the
 * caller's to free (hipFreeSpmat).  spmvHipInit() may be called again afterwards. */
int spmvHipFinalize(void);
/* number of visible devices, or -1 */
int spmvHipDeviceCount(void);
/* Stream (hipStream_t passed as void*) used by all later launches/copies of the
 * calling process; NULL = the default stream.  The library uses a stream only INSIDE the calls made while it is set (or
 * passed): it may be destroyed afterwards without telling the library (the two-phase kernel's product workspace is handed
 * from stream to stream through an event recorded behind each use, never through the previous stream). */
int spmvHipSetStream(void* stream);
/* (With spmvHipSetSync(0) a launcher whose format exists only enqueues kernels on this stream -- no allocation, no
 * synchronisation, no timing events; the two-phase launcher records its one hand-over event unless the stream is being
 * captured -- so a solver's inner loop can be captured into a HIP graph and replayed:
 * tests/test_gpu_parity.py::test_launchers_capture_into_a_hip_graph.  A captured two-phase launch uses the device's product
 * workspace whenever the graph is replayed, which the library cannot see: keep replays in stream order with, or
 * synchronised against, two-phase launches of OTHER streams.)
 * Every launcher checks on the host what it can: the handle (kind, magic), NULL x / y (refused: a NULL would be a GPU page
 * fault in every lane); the EXTENT of x and y is the caller's promise, as in the reference. */
/* sync != 0 (default): every SpMV launcher waits for completion before it
 * returns and stores the device time in `ElapsedInternal`-style seconds
 * retrievable with spmvHipLastKernelSeconds() -- the behaviour of the
 * reference drivers (launch; cudaDeviceSynchronize; main.cu:233-238).
 * sync == 0: launchers only enqueue (for timed loops and graph capture). */
int spmvHipSetSync(int sync);
double spmvHipLastKernelSeconds(void);
/* launch shape of the most recent SpMV launcher call */
int spmvHipLastLaunch(spmvDim3* grid, spmvDim3* block);
int spmvHipDeviceSynchronize(void);

/* ------------------------------------------------------------- dense vectors */
int spmvHipVecAlloc(double** dVec, size_t n);
int spmvHipVecFree(double* dVec);
int spmvHipVecUp(double* dVec, const double* hVec, size_t n);
int spmvHipVecDown(double* hVec, const double* dVec, size_t n);
/* fill with a 64-bit pattern (e.g. a NaN payload to poison y before a launch) */
int spmvHipVecFill(double* dVec, size_t n, uint64_t pattern);

/* raw device bytes (device-format index arrays built on the GPU) */
int spmvHipMalloc(void** dPtr, size_t bytes);
int spmvHipFree(void* dPtr);
int spmvHipMemcpyUp(void* dDst, const void* hSrc, size_t bytes);
int spmvHipMemcpyDown(void* hDst, const void* dSrc, size_t bytes);

/* ------------------------------------------------------------- refused allocations (for tests)
 * These two exist for tests.  Every device allocation and release of the library -- handles, formats, schedules,
 * workspaces, temporaries, and the vectors and bytes handed out above -- goes through one place that keeps a ledger:
 *   live, liveBytes   what the library holds on the device now (allocations and their bytes as asked for)
 *   peakBytes         the most it held at once since the process started
 *   calls             allocations asked for since the last spmvHipAllocRefuse
 *   refused           how many of those were refused on purpose
 *   badFrees          releases of a pointer the ledger does not hold: a second release, or memory that came from
 *                     elsewhere (such a pointer is still passed on to the runtime, whose answer decides the call)
 * spmvHipAllocRefuse(n, fromThenOn) sets calls and refused to 0 and, with n >= 0, makes allocation number n from now
 * (0-based) fail: that one alone, or with fromThenOn != 0 that one and every later one, until spmvHipAllocRefuse(-1, 0).
 * A refused allocation is a real refusal of the runtime -- it is asked for 2^62 bytes -- so the caller sees the
 * runtime's own error code and the runtime's own sticky last error.  No environment variable arms it.  Both work
 * before spmvHipInit.
 *
 * What a failed device allocation leaves (tests/test_gpu_alloc_refusals.py refuses every allocation of every call below
 * in turn).  For every call: EXIT_FAILURE, at least one "libspmvhip" line on stderr, no sticky runtime error -- the
 * next, unrelated call is judged on its own --, the source handles untouched (values, built formats, selections), and
 * the same call made again succeeds with the result it would have given at first.  And by family:
 *   a call that makes a handle (spMatCpyCSR / ELL, spmvHipAdoptCSR, spmvHipCsrToEll, spmvHipCsrTranspose, ...Permute,
 *     spmvHipSpGEMM, spmvHipCsrAdd, spmvHipCsrFilter, spmvHipCooAssemble, spmvHipFsaiSetup, the three spmvHipAmgSetup*): the destination handle
 *     and info are not written, and nothing the call allocated is still held;
 *   a format build (spmvHipBuildTiles / Stripes / Sell and their *Opt forms, the first call of a format's launcher): the
 *     handle stays a live CSR handle without that format, nothing of the format is held.  The device's product workspace of
 *     the two-phase kernel (8 B per entry of the largest matrix built), once grown, stays the library's until
 *     spmvHipFinalize;
 *   the selections of hipSpMVRowsCSR / hipSpMVWarpPerRowCSR / hipSpMVAutoCSR: the one exception to EXIT_FAILURE.  A
 *     candidate whose format cannot be built is skipped; with nothing to allocate the call still answers, with the kernel
 *     that needs no memory of its own;
 *   spmvHipUpdateValues, spmvHipValuesChanged and the refreshes (spmvHipTransposeRefresh, ...PermuteRefresh,
 *     ...SpGEMMRefresh, ...CsrAddRefresh, ...CsrFilterRefresh, spmvHipCooAssembleRefresh, spmvHipFsaiRefresh, spmvHipAmgRefresh): the handle stays live with its pattern,
 *     its addresses and every built format; info is not written; the CSR values may be the new ones while a built format
 *     or a coarser level still holds the old ones.  CALL AGAIN before the handle is used: the repeated call completes it;
 *   the first hipSpTRSVCSR / hipSpTRSMCSR of a triangle, spmvHipTriAnalyse: x is not written, no schedule is left;
 *   hipSpILU0CSR: AS untouched bit for bit, and the lower triangle's schedule, if it was made, stays on the handle.  One
 *     allocation comes after the factorisation (the unit flag of the new values): when that fails the line says "the
 *     factors are in place", AS holds the complete factors, and the same call made again finishes the handle without
 *     factorising a second time (a value update or a refresh in between makes it an ordinary factorisation again; see
 *     hipSpILU0CSR's own comment for a caller who rewrites an adopted dAS);
 *   spmvHipDot / MultiDot / BlockDot: the result is not written, the dot workspace keeps the size it had;
 *   hipSpCGCSR, hipSpBiCGStabCSR, hipSpGMRESCSR (every allocation comes before the loop): x and info are not written; a
 *     schedule that was made on dM stays there;
 *   hipSpLanczosCSR, hipSpDavidsonCSR (every allocation comes before the loop): dX, theta, res and info are not written;
 *   spmvHipBlockResidual: dR and dNorm2 are not written, the dot workspace keeps the size it had;
 *   spmvHipColourCSR, spmvHipAggregateCSR: info is not written, nothing is held; dColour / dPerm / dAgg may have been
 *     written in part and hold nothing to rely on;
 *   spmvHipAmgSetSmoother, spmvHipAmgSetGaussSeidel, spmvHipAmgSetBlockWidth: everything new is made before anything old
 *     is dropped -- the hierarchy keeps its smoother, its sweep counts and its block width, the cycle gives the bits it
 *     gave before, and nothing the call allocated is still held. */
typedef struct {
    ulong live, liveBytes, peakBytes, calls, refused, badFrees;
} spmvAllocStats;
int spmvHipAllocRefuse(long n, int fromThenOn);
int spmvHipAllocStats(spmvAllocStats* stats);

/* ------------------------------------------------------------- matrix upload */
/* Host CSR -> device (cudaUtils.cu:20-55).  `dMat` is caller-owned host memory
 * that becomes the device handle.  Column ids are narrowed to 32 bit, row
 * pointers to 32 bit when NZ < 2^32; row blocks for the LDS-stream kernel are
 * computed here.  host->RL may be NULL. */
int spMatCpyCSR(spmat* host, spmat* dMat);
/* Host ELL -> device (cudaUtils.cu:56-98).  Accepts the row-major matrix the
 * loader produces, or the output of ellTranspose() (recognised the same way
 * the reference kernels do: after transposition M holds the slot count and
 * MAX_ROW_NZ the row count, sparseUtils.c:168-171) -- pass `transposed` = 1 for
 * the latter.  Pitch = row length rounded up to 64 elements; pitchJA/pitchAS
 * are stored in elements as the reference does (cudaUtils.cu:81-83).  The
 * reference's field swap loses the column count of a transposed matrix; this
 * repo's ellTranspose() keeps it in the (otherwise unused) host field pitchJA
 * and the upload checks every column id against it (0 = unknown, unchecked). */
int spMatCpyELL(spmat* host, spmat* dMat);
int spMatCpyELLTransposed(spmat* hostT, spmat* dMat);
/* Device-side CSR -> ELL of an uploaded matrix (slots = its longest row, row
 * lengths kept): transposed = 0 gives the row-major handle spMatCpyELL(ell)
 * would, 1 the column-major one of ellTranspose + spMatCpyELL.  ELL size
 * guard: the reference's loader refuses an ELL copy above a fixed number of
 * padded cells (parser.c:223-232); here the copy is refused (EXIT_FAILURE, no
 * allocation attempted) when it does not fit the device memory that is free. */
int spmvHipCsrToEll(spmat* dCsr, int transposed, spmat* dEll);
/* ------------------------------------------------------------- transposed products */
/* The transpose of a device CSR handle, built on the device as a new, independent CSR handle: for y = A^T x (BiCG, QMR,
 * LSQR / CGNR, adjoints and gradients such as A^T (A x - b), PageRank pulls along in-edges).  DESIGN.md section 16.
 * spmvHipCsrTranspose writes into dAT a CSR handle of A^T: dAT->M = A.N, dAT->N = A.M, the same NZ.  The caller owns it
 *   and frees it with hipFreeSpmat.
 *   Order: STABLE.  Row j of A^T holds the entries of column j of A in their CSR position order -- ascending source row,
 *   and within a row the stored order -- unsorted rows and repeated (i, j) pairs included.  JA of dAT holds the source
 *   row ids (u32), AS the values; the row pointers are 4 bytes.
 *   Every CSR entry point works on dAT unchanged (both selections, variants 0-2, the explicit two-phase / stripes / SELL
 *   launchers, hipSpMMRowsCSR, graph capture, spmvHipUpdateValues).  hipSpMVRowsCSR(dAT, x, y) gives the bits of the
 *   serial scatter loop, on every candidate of its selection:
 *       y = +0.0;  for i in 0..M-1: for p in IRP[i]..IRP[i+1]-1: y[JA[p]] += AS[p] * x[i]
 *   i.e. sgemvSerial on the stable transpose: its rows have non-decreasing column ids, which the serial-order selection
 *   counts as sorted, and the deterministic two-phase and stripes forms keep the stored order of equal columns.
 *   Sources: spMatCpyCSR / spmvHipAdoptCSR handles with 4- or 8-byte row pointers, unit-value handles included.  dAT runs
 *   its own unit detection (spmvHipSetUnitValues).
 *   Ordering: the build runs on the library stream, after what is already enqueued there (an AS just written there), and
 *   returns with dAT complete.  It allocates: not capturable.
 *   Device memory of dAT: 4 (A.N + 1) B of row pointers; 16 B/nnz (JA 4, AS 8, and the source-position map 4, kept for
 *   spmvHipTransposeRefresh); the row blocks.  Build temporaries (4 B/nnz of source rows, the sort's workspace) are freed
 *   before the call returns.
 * spmvHipTransposeRefresh gathers dAT's values from dA's value array as it is on the device (for an adopted source the
 *   caller's array), then does exactly what spmvHipValuesChanged(dAT) does: the unit detection, every built format in both
 *   forms, the unit transition rules of spmvHipUpdateValues.  Selections and device addresses stay, so a graph captured on
 *   dAT replays with the new values; spmvHipLastUpdateInfo(dAT) reports the call.  Ordering as spmvHipValuesChanged.
 * Source identity: every device handle has a process-unique id, and dAT records its source's.  A refresh from any other
 *   handle is refused, even one of the same shape or one that reuses a freed source's memory.  dAT keeps no pointer to
 *   dA: freeing either first is safe.
 * Refused with a message and EXIT_FAILURE, dAT untouched: NULL pointers, or a handle that is not live; dAT == dA; ELL
 *   handles, spmvHipCsrToEll's included; A.NZ >= IRP32_LIMIT (2^32 - 65536: the map and the positions are 32-bit, the
 *   limit of the two-phase and stripes formats); A.N >= 2^32 - 1 (the rows of A^T must fit the device format); a refresh
 *   of a handle that is not a transpose, or from a handle that is not its source. */
int spmvHipCsrTranspose(spmat* dA, spmat* dAT);
int spmvHipTransposeRefresh(spmat* dAT, spmat* dA);
/* ------------------------------------------------------------- triangular solves */
/* x = T^-1 b for the lower or upper triangle T of a square device CSR handle (M == N): Gauss-Seidel / SGS sweeps, SOR,
 * ILU(0) / IC(0) preconditioners, back-substitution.  DESIGN.md section 17.  The solve writes the bits of this loop, in
 * IEEE double with no FMA contraction (the library is built with -ffp-contract=off):
 *     lower: for i = 0, 1, ..., M-1            upper: for i = M-1, M-2, ..., 0
 *         acc = +0.0
 *         for p in IRP[i] .. IRP[i+1]-1   (stored order)
 *             j = JA[p]
 *             if (lower ? j < i : j > i):  acc += AS[p] * x[j]      -- one rounding for the product, one for the add
 *         x[i] = STORED ? (b[i] - acc) / AS[diagPos[i]] : (b[i] - acc)
 *   Entries on the other side of the diagonal are IGNORED: the whole matrix A may be passed, for a forward or backward
 *   Gauss-Seidel sweep on its triangle.  Unsorted rows and repeated (i, j) pairs are allowed; every stored strict-triangle
 *   entry is added, in stored order.  One handle may hold an ILU(0) pair (strictly lower L with unit diagonal, U with the
 *   diagonal): hipSpTRSVCSR(LOWER, UNIT) then hipSpTRSVCSR(UPPER, STORED) applies the preconditioner.
 *   STORED: every row holds exactly one entry with j == i, diagPos[i].  UNIT: diagonal entries are ignored, stored or not.
 *   A stored diagonal value of 0.0 is not an error: x[i] is then +-Inf or NaN as the loop gives, and propagates as the
 *   loop propagates it.  Unit-value handles (spmvHipUnitValue) take the value from a register: c * x rounds as AS[p] * x.
 *   dB == dX (in place) is allowed: a row reads b only at its own index, writes x only at its own index, and reads x only
 *   at rows that are already final.
 * Analysis: level sets of the triangle's pattern, one schedule per triangle kept on the handle; spmvHipTriAnalyse builds it
 *   (a no-op when it exists), and the first solve of an unanalysed triangle does.  Synchronous, allocates (not capturable).
 *   spmvHipUpdateValues, spmvHipValuesChanged and spmvHipTransposeRefresh keep it (the solve reads AS live); hipFreeSpmat
 *   frees it.  Device memory kept: 8 B per row and 4 B per level.  Build temporaries (16 B/nnz, 16 B/row, the sorts'
 *   workspace) are freed before the call returns.  The runs' row threshold T is 256 (spmvHipSetVariant("hipSpTRSVCSR",
 *   T), 0 <= T <= 65536, sets it for later analyses; 0: no runs).
 * Solve: kernels only, on the library stream, one launch per wide level and one per run of thin levels; no allocation and
 *   no host sync once the triangle is analysed, so it can be captured into a graph after spmvHipTriAnalyse.  With
 *   spmvHipSetSync(1) it waits and sets spmvHipLastKernelSeconds (the whole solve) and spmvHipLastLaunch (the last launch);
 *   with spmvHipSetSync(0) it only enqueues.  M = 0 succeeds and writes nothing.
 * Refused with a message and EXIT_FAILURE, x untouched: NULL pointers, or a handle that is not live; ELL handles,
 *   spmvHipCsrToEll's included; M != N; an unknown uplo or diag; NZ >= IRP32_LIMIT or M >= 2^31 (positions and rows are
 *   32-bit); STORED when firstBadDiag >= 0 (the message names the row); dB and dX overlapping without being equal.
 * spmvHipTriInfo: the schedule of one triangle, all zeros (and firstBadDiag 0) when it has not been analysed. */
#define SPMV_TRI_LOWER   0
#define SPMV_TRI_UPPER   1
#define SPMV_DIAG_STORED 0
#define SPMV_DIAG_UNIT   1
typedef struct {
    ulong  levels;          /* 0: this triangle has not been analysed                               */
    ulong  maxLevelRows;    /* rows of the widest level                                              */
    ulong  launches;        /* kernel launches one solve enqueues                                    */
    ulong  fusedLevels;     /* levels solved inside single-workgroup runs                            */
    ulong  longRows;        /* rows on the wavefront-per-row path                                    */
    long   firstBadDiag;    /* -1, or the first row without exactly one stored diagonal entry        */
    int    analyses;        /* analyses run on this handle for this triangle (stays 1 across updates) */
    double analysisMs;      /* host wall time of the last analysis                                   */
    size_t bytes;           /* device memory the schedule keeps                                      */
} spmvTriInfo;
int spmvHipTriAnalyse(spmat* dA, int uplo);
int hipSpTRSVCSR(spmat* dA, int uplo, int diag, const double* dB, double* dX);
int spmvHipTriInfo(spmat* dA, int uplo, spmvTriInfo* info);
/* hipSpTRSMCSR: X = T^-1 B for a block of k right-hand sides, all columns in one pass over the triangle.  DESIGN.md section
 * 26.  B and X are M x k on the device, each in its own layout with its own leading dimension, exactly those of
 * hipSpMMRowsCSR below: SPMV_DENSE_ROW_MAJOR (0, element (i, c) at P[i*ld + c], ld >= k) or SPMV_DENSE_COL_MAJOR (1,
 * element (i, c) at P[c*ld + i], ld >= M).
 *   Bits: column c of X has the bits of hipSpTRSVCSR(dA, uplo, diag, B[:, c], .), i.e. of the loop above applied per
 *   column: rows in order, strict-triangle products rounded and added in stored order from +0.0, entries outside the
 *   triangle skipped (never added as 0.0), then (b - acc), divided by the stored diagonal unless diag is UNIT.  Unsorted rows
 *   and repeated pairs behave as in the single solve; a zero stored diagonal gives +-Inf or NaN and propagates as in the
 *   loop; unit-value handles take the value from a register.  Columns are independent: an Inf or NaN in one column never
 *   reaches another.
 *   Width: any k >= 1.  Columns are taken in panels of at most 16, and all panels of a level go in ONE launch: a k-column
 *   solve enqueues exactly spmvTriInfo.launches launches, whatever k is.  (k = 1 with unit strides runs the single solve.)
 *   In place: dB == dX with equal layout and equal leading dimension is allowed (a row reads B only at its own (i, c) and
 *   writes X only there).  Any other overlap of the two address spans is refused, the same pointer with another layout or
 *   leading dimension included; the check is made on the host.
 *   Padding: elements of X outside the M x k block are never written (nor read), those of B never read.
 *   Schedule: the TriSchedule of the handle, shared with hipSpTRSVCSR: the first call on an unanalysed triangle analyses
 *   it, a later hipSpTRSVCSR reuses that analysis and the other way round (spmvTriInfo.analyses stays 1);
 *   spmvHipUpdateValues, spmvHipValuesChanged and spmvHipTransposeRefresh keep it, values are read live.
 *   Launch: kernels only, on the library stream; no allocation and no host sync once the triangle is analysed, so the
 *   solve can be captured into a graph after spmvHipTriAnalyse.  With spmvHipSetSync(1) it waits and sets
 *   spmvHipLastKernelSeconds (the whole solve) and spmvHipLastLaunch (the last launch); with spmvHipSetSync(0) it only
 *   enqueues.  M = 0 succeeds and writes nothing.
 * Refused with a message and EXIT_FAILURE, X untouched: NULL pointers, or a handle that is not live; ELL handles; M != N;
 *   an unknown uplo, diag or layout; k = 0; a leading dimension too small for its layout; NZ >= IRP32_LIMIT or M >= 2^31;
 *   STORED when firstBadDiag >= 0 (the message names the row); a handle with entries and no value array that is not
 *   unit-value; the overlaps above; a multigrid hierarchy handle. */
int hipSpTRSMCSR(spmat* dA, int uplo, int diag, unsigned k, const double* dB, size_t ldb, int bLayout,
                 double* dX, size_t ldx, int xLayout);
/* Triangular solves by Jacobi sweeps: a fixed number S of sweeps on the triangle in place of the exact solve, for use as a
 * preconditioner (iterative sparse triangular solves, Anzt, Chow and Dongarra).  DESIGN.md section 40.  A sweep has no
 * dependence between rows: it is one launch, and no level sets are built.  The solve writes the bits of this loop, in IEEE
 * double with no FMA contraction:
 *     hipSpTRSVSweepsCSR(dA, uplo, diag, S, b, x):      T = the strict lower / upper triangle of dA, d_i = AS[diagPos[i]]
 *         x0[i] = STORED ? b[i] / d_i : b[i]                                  for every i
 *         for s = 1 .. S:                                                    (rows in any order: they read only x(s-1))
 *             for every i:
 *                 acc = +0.0
 *                 for p in IRP[i] .. IRP[i+1]-1   (stored order)
 *                     j = JA[p];  if (lower ? j < i : j > i):  acc += AS[p] * x(s-1)[j]     -- one rounding each, no FMA
 *                 x(s)[i] = STORED ? (b[i] - acc) / d_i : (b[i] - acc)
 *         x = x(S)
 *   1. Entries outside the strict triangle are skipped, never added as 0.0 (-0.0 + 0.0 is +0.0).  Unsorted rows and repeated
 *      (i, j) pairs are allowed; every stored strict-triangle entry is added, in stored order.
 *   2. STORED needs exactly one diagonal entry per row, else the call is refused and the message names the row.  A zero
 *      stored diagonal gives +-Inf or NaN exactly as the loop does.
 *   3. Unit-value handles take the value from a register, as in hipSpTRSVCSR.
 *   4. Consequence: x(S)[i] is the exact solution's x[i], bit for bit, on every row i whose level is at most S (induction on
 *      the level: such a row reads only rows of lower levels, which are final from sweep level(j) <= S - 1 on, in the same
 *      stored order as the exact loop).  So for S >= levels - 1 of that triangle (spmvTriInfo.levels) x has the bits of
 *      hipSpTRSVCSR.  A row of level 0 has acc = +0.0, and b - (+0.0) is b bit for bit.  S = 0 is the diagonal scaling.
 *   5. dB == dX (in place) is allowed: every intermediate iterate lives in the plan's workspace and only the last sweep
 *      writes x, reading b at its own index.  Any other overlap is refused.
 *   6. S above SPMV_TRI_SWEEPS_MAX (4096) is refused.
 *   7. hipSpTRSMSweepsCSR: the argument list of hipSpTRSMCSR plus S; column c of X has the bits of the single sweep solve on
 *      column c of B; both layouts and leading dimensions; padding is never written (nor read); columns go in panels of at
 *      most 16 inside ONE launch per sweep, so the launch count does not depend on k.  In place as hipSpTRSMCSR.
 *   8. As a preconditioner (spmvHipTriSetApply(dM, SPMV_TRI_APPLY_SWEEPS, S_L, S_U, width)): z = U~^-1 (L~^-1 r) with S_L
 *      lower sweeps (UNIT) and S_U upper sweeps (STORED) wherever a Krylov solve takes this handle as dM -- hipSpCGCSR,
 *      hipSpBiCGStabCSR, hipSpGMRESCSR and, with width >= k, the block solves -- whose launch counters count the sweep launches;
 *      no level sets are analysed for such a dM.  For the ILU(0) factors of a symmetric A with S_L == S_U = S the operator is
 *      M^-1 = P^T D^-1 P, P = sum_{j <= S} (-strict L)^j: symmetric, and positive definite whenever the factored diagonal is
 *      positive, so it is a CG preconditioner.  Unequal counts are for BiCGStab and GMRES only; this is not checked, as the
 *      symmetry of A is not.  Strong couplings need more sweeps (DESIGN.md section 40 has the counts).  SPMV_TRI_APPLY_EXACT
 *      (the default) gives the exact solves and their bits again; the plan stays.
 * Plan: spmvHipTriSweepsPrepare(dA, blockWidth) builds it (blockWidth 0: one column; a larger width than the plan's widens
 *   the workspace, a smaller one is a no-op): the diagonal's places and two M x width iterates, 4 B + 16 B x width per row.
 *   Synchronous, allocates (not capturable).  The first sweep solve of an unprepared handle prepares it for its own width.
 *   spmvHipUpdateValues, spmvHipValuesChanged, hipSpILU0CSR and every refresh that keeps the handle's pattern --
 *   spmvHipTransposeRefresh, spmvHipPermuteRefresh, spmvHipSpGEMMRefresh, spmvHipCsrAddRefresh, spmvHipCsrFilterRefresh and
 *   spmvHipCooAssembleRefresh -- keep it at the same addresses with `prepares` unchanged, and keep the apply mode and its
 *   sweep counts (the sweeps read AS live); only a widening moves the workspace, never diagPos; hipFreeSpmat frees it.
 * Solve: kernels only, on the library stream: S launches (UNIT; S + 1 for S == 1 in place; S == 0: one copy, none in place),
 *   S + 1 (STORED); no allocation and no host sync once prepared, so it can be captured into a graph.  spmvHipSetSync,
 *   spmvHipLastKernelSeconds and spmvHipLastLaunch as for hipSpTRSVCSR.  M = 0 succeeds and writes nothing.
 * Refused with a message and EXIT_FAILURE, outputs and handle untouched: what hipSpTRSVCSR / hipSpTRSMCSR refuse; S above
 *   the cap; an unknown mode; k above the prepared width.
 * spmvHipTriSweepsInfo: all zeros while the handle has no plan. */
#define SPMV_TRI_APPLY_EXACT  0
#define SPMV_TRI_APPLY_SWEEPS 1
#define SPMV_TRI_SWEEPS_MAX   4096
typedef struct {
    int      mode;          /* SPMV_TRI_APPLY_EXACT | SPMV_TRI_APPLY_SWEEPS: how a Krylov solve applies this handle as dM */
    unsigned lowerSweeps;   /* S_L and                                                                               */
    unsigned upperSweeps;   /* S_U of one application in SWEEPS mode                                                 */
    unsigned width;         /* columns the workspace holds; 0: no plan                                               */
    ulong    solveLaunches; /* kernel launches the last sweep solve enqueued                                         */
    ulong    applyLaunches; /* launches of one application in SWEEPS mode: S_L + S_U, + 1 when one of them is 0; EXACT: 0 */
    long     firstBadDiag;  /* -1, or the first row without exactly one stored diagonal entry                        */
    int      sorted;        /* every row ascends strictly and holds one diagonal entry (the ILU(0) precondition)     */
    int      prepares;      /* builds and widenings of the plan (stays 1 across value updates)                       */
    size_t   bytes;         /* device memory the plan keeps                                                          */
    const uint32_t* diagPos;    /* the plan's device arrays (for address checks; NULL without a plan): the diagonal's places */
    const double*   workspace;  /* ... and the two M x width iterates                                                 */
} spmvTriSweepsInfo;
int spmvHipTriSweepsPrepare(spmat* dA, unsigned blockWidth);
int hipSpTRSVSweepsCSR(spmat* dA, int uplo, int diag, unsigned sweeps, const double* dB, double* dX);
int hipSpTRSMSweepsCSR(spmat* dA, int uplo, int diag, unsigned sweeps, unsigned k, const double* dB, size_t ldb, int bLayout,
                       double* dX, size_t ldx, int xLayout);
int spmvHipTriSetApply(spmat* dA, int mode, unsigned lowerSweeps, unsigned upperSweeps, unsigned blockWidth);
int spmvHipTriSweepsInfo(spmat* dA, spmvTriSweepsInfo* info);
/* ------------------------------------------------------------- incomplete factorisation */
/* hipSpILU0CSR overwrites the values of a square device CSR handle with its ILU(0) factors, in place: the strictly lower
 * part becomes L (unit diagonal, not stored), the diagonal and the upper part U, so that hipSpTRSVCSR(LOWER, UNIT) then
 * hipSpTRSVCSR(UPPER, STORED) on the same handle applies the preconditioner.  DESIGN.md section 18.  AS ends with the bits
 * of this loop, in IEEE double with no FMA contraction (the library is built with -ffp-contract=off):
 *     for i = 0, 1, ..., M-1
 *         for p = IRP[i] .. diagPos[i]-1                 -- k = JA[p] < i, ascending
 *             k = JA[p]
 *             AS[p] = AS[p] / AS[diagPos[k]]             -- row k is final
 *             for q = p+1 .. IRP[i+1]-1                   -- j = JA[q] > k, ascending
 *                 if row k stores column JA[q] at position r:
 *                     AS[q] = AS[q] - AS[p] * AS[r]      -- one rounding for the product, one for the subtraction
 *   Preconditions (of the pattern; checked once per handle, the answer kept across value updates): every row's columns are
 *   strictly ascending (sorted, no repeated column) and every row holds exactly one diagonal entry.
 *   Zero pivot: a factored diagonal of +-0.0 is not an error (as in hipSpTRSVCSR); later rows get +-Inf or NaN exactly as
 *   the loop gives them, and spmvIluInfo.zeroPivot names the smallest such row (cuSPARSE's csrilu02_zeroPivot).
 *   Afterwards the handle is refreshed as by spmvHipValuesChanged: unit detection runs again (a pattern handle stops being
 *   unit), built formats take the new values, the selections stay; hipSpMVRowsCSR on it gives sgemvSerial of the L\U
 *   values.  For a spmvHipAdoptCSR handle the caller's dAS is overwritten.
 *   Schedule: the lower triangle's level sets (spmvHipTriAnalyse(dA, SPMV_TRI_LOWER)), built by this call when missing and
 *   never a second time: spmvTriInfo.analyses stays 1 across refactorisations.  Rows of one level are factored in parallel,
 *   each by a group of lanes (16; spmvHipSetVariant("hipSpILU0CSR", 8 | 16 | 64)), in one launch per wide level and one
 *   single-workgroup launch per run of thin levels, on the library stream.
 *   Synchronous (it reads the zero-pivot word back and refreshes the handle), allocates a few words: not capturable.
 *   M = 0 succeeds.
 * Refused with a message and EXIT_FAILURE, AS untouched bit for bit: NULL, or a handle that is not live, or one with no
 *   value array; ELL handles, spmvHipCsrToEll's included (sharded matrices are no spmat handles); M != N; NZ >= IRP32_LIMIT
 *   or M >= 2^31 (the solve's limits); a row whose columns are not strictly ascending, or a row without exactly one
 *   diagonal entry (the message names the row; spmvIluInfo.firstBadRow is the smaller of the two).
 *   A failed device allocation is another matter ("refused allocations" above, hipSpILU0CSR's line): AS is untouched, or
 *   -- the message then says "the factors are in place" -- holds the complete factors, and the same call made again
 *   finishes the handle without factorising twice.  The library forgets that state whenever IT rewrites AS
 *   (spmvHipUpdateValues, spmvHipValuesChanged, a refresh of a derived handle, failed or not).  A caller who rewrites an
 *   adopted dAS after such a failure must call spmvHipValuesChanged before the next hipSpILU0CSR: without it the call
 *   would take the new values for the factors it is about to finish.
 * spmvHipIlu0Info: what the last factorisation of the handle did (all zeros, zeroPivot and firstBadRow -1, before one). */
typedef struct {
    long   zeroPivot;       /* -1, or the smallest row whose factored diagonal is +-0.0      */
    long   firstBadRow;     /* -1, or the first row refused (unsorted / repeated / diagonal) */
    ulong  levels;          /* levels of the lower schedule the factorisation ran by         */
    ulong  launches;        /* kernel launches of one factorisation                          */
    ulong  longRows;        /* rows that took the long-row path                              */
    int    factorisations;  /* on this handle                                                */
    double ms;              /* host wall time of the last call                               */
} spmvIluInfo;
int hipSpILU0CSR(spmat* dA);
int spmvHipIlu0Info(spmat* dA, spmvIluInfo* info);
/* ------------------------------------------------------------- approximate-inverse preconditioner (FSAI) */
/* spmvHipFsaiSetup makes the factorised sparse approximate inverse of a square device CSR handle (Kolotilina-Yeremin): a
 * sparse lower-triangular G with G^T G ~ A^-1, as a live CSR handle dG of its own.  M^-1 v = G^T (G v) is two serial-order
 * SpMVs: no level sets, no analysis, no dependence between rows.  G A G^T has a unit diagonal, so G contains the Jacobi
 * scaling, and M^-1 is symmetric positive definite by construction: CG may use it.  DESIGN.md section 38.
 *   dA: only its LOWER triangle including the diagonal is ever read; symmetry is the caller's promise, as it is for CG.
 *   dS: a pattern handle of the same size (its values are not read), or NULL for dA itself.  The caller sets the quality by
 *   the pattern: tril(A), tril(A A) by spmvHipSpGEMM, a thresholded one by spmvHipCsrFilter.  dS need not outlive the call.
 *   Both must have strictly ascending rows (sorted, no repeated column): hipSpILU0CSR's check, made once per handle.
 * For row i, P = (p_0 < p_1 < ... < p_{n-1} = i) is the columns j < i that row i of dS stores, then i itself, whether or not
 * dS stores the diagonal.  Row i of G stores exactly the columns P, ascending, the diagonal last.  Its values are
 * g[0 .. n-1] of this loop, in IEEE double with no FMA contraction and with sqrt and / correctly rounded:
 *     B[s][t] = the value of the stored entry (p_s, p_t) of dA, +0.0 if row p_s stores no column p_t      (0 <= t <= s < n)
 *     for k = 0 .. n-1:
 *         if !(B[k][k] > 0) or B[k][k] == +inf:  the row is BAD, stop
 *         B[k][k] = sqrt(B[k][k])
 *         for s = k+1 .. n-1:  B[s][k] = B[s][k] / B[k][k]
 *         for t = k+1 .. n-1, s = t .. n-1:  B[s][t] = B[s][t] - B[s][k]*B[t][k]     -- the product rounded, then the difference
 *     y[n-1] = (1.0 / B[n-1][n-1]) / B[n-1][n-1]
 *     for t = n-2 down to 0:
 *         acc = +0.0;  for s = n-1 down to t+1:  acc = acc + B[s][t]*y[s]
 *         y[t] = (0.0 - acc) / B[t][t]
 *     d = sqrt(y[n-1]);  if !(d > 0) or d == +inf: the row is BAD
 *     g[t] = y[t] / d                                                                    (t = 0 .. n-1)
 *     BAD row: g[0 .. n-2] = +0.0, g[n-1] = 1.0
 *   Both halves are the right-looking forms: every entry of B receives its updates one at a time in ascending k, and every
 *   acc receives its terms in descending s, whichever lane does the work.  (The Crout form sums first and subtracts once:
 *   other bits.)  The group of lanes that computes a row (4, 16 or 64; spmvFsaiOpts.lanesPerRow forces one, 0 is the
 *   built-in choice by the mean row of G) does not change a bit.
 *   A pattern row with n > SPMV_FSAI_MAX_ROW is refused, the message naming the first such row: filter the pattern.
 *   A BAD row is NOT a refusal: the handle is made, and info.badRows / info.firstBadRow (-1: none) report it.
 *   M = 0 succeeds with no kernel.
 * dG is an ordinary live CSR handle (SpMV, transpose, product, filter, spmvHipCsrToCoo take it: G A G^T can be formed with
 *   the public product) that privately owns G^T -- the handle spmvHipCsrTranspose would make of G -- and one M-vector of
 *   workspace; hipFreeSpmat(dG) frees all three.  Synchronous, allocates: not capturable.  dG is to be read, not written:
 *   after a direct write into it (spmvHipUpdateValues, spmvHipValuesChanged, hipSpILU0CSR) or a spmvHipValuesF32 call on it the
 *   owned G^T and the storage setting no longer match G, and what spmvHipFsaiApply and a solver compute with it is undefined
 *   until the next spmvHipFsaiRefresh; its values change through spmvHipFsaiRefresh, its f32 forms through spmvHipFsaiSetStorage.
 * spmvHipFsaiRefresh(dG, dA): dA -- the handle of the setup -- has new values on the same pattern at the same addresses.  The
 *   values of G are computed again in place over the setup's columns, G^T takes them through its map, and both are refreshed
 *   as by spmvHipValuesChanged.  IRP, JA and AS keep their addresses.
 * spmvHipFsaiApply(dG, dR, dZ): z = G^T (G r), both products serial-order SpMV (sgemvSerial's bits), through the handle's
 *   workspace; dR == dZ is allowed, any other overlap is refused.  Kernels only after the first call (which chooses the
 *   kernels of G and G^T); spmvHipSetSync as for the launchers.
 * spmvHipFsaiTranspose(dG, dGT): *dGT becomes a borrowed view of the G^T the handle owns (dev = NULL: its arrays stay dG's).
 * spmvHipFsaiInfo: what the setup or the last refresh did.
 * As dM of hipSpCGCSR / hipSpBiCGStabCSR / hipSpGMRESCSR and the block solvers: see there.
 * Refused with a message and EXIT_FAILURE, every check before the first write -- a setup does not write dG or info, a
 *   refresh leaves dG as it was: NULL dA or dG (dR, dZ); dG == dA or dG == dS; handles that are not live; ELL handles;
 *   M != N; NZ >= IRP32_LIMIT or M >= 2^31; dS of another size than dA; a dA without a value array; lanesPerRow that is none
 *   of 0, 4, 16, 64; a row of dA or dS that is not strictly ascending; a pattern row above SPMV_FSAI_MAX_ROW; a dG that
 *   spmvHipFsaiSetup did not make, or (refresh) not from this dA.  A failed device allocation: "refused allocations" above. */
#define SPMV_FSAI_MAX_ROW 64
typedef struct {
    unsigned lanesPerRow;   /* 0 = the built-in choice; 4, 16 or 64 forces the group that computes a row */
} spmvFsaiOpts;
typedef struct {
    ulong  nnz;             /* entries of G                                                   */
    ulong  maxRow;          /* its longest row                                                */
    ulong  badRows;         /* rows that got the identity row                                 */
    long   firstBadRow;     /* -1, or the smallest of them                                    */
    ulong  launches;        /* kernel launches of the setup's passes, or of the last refresh  */
    ulong  setups;          /* the setup and every refresh since                              */
    double ms;              /* host wall time of the last call                                */
} spmvFsaiInfo;
int spmvHipFsaiSetup(spmat* dA, spmat* dS, const spmvFsaiOpts* opts, spmat* dG, spmvFsaiInfo* info);
int spmvHipFsaiRefresh(spmat* dG, spmat* dA, spmvFsaiInfo* info);
int spmvHipFsaiApply(spmat* dG, const double* dR, double* dZ);
int spmvHipFsaiTranspose(spmat* dG, spmat* dGT);
int spmvHipFsaiInfo(spmat* dG, spmvFsaiInfo* info);
/* The factor stored in single precision.  spmvHipFsaiSetStorage(dG, SPMV_STORAGE_F32) builds the
 * single-precision value form (spmvHipValuesF32, below) on G and on the G^T the factor owns; SPMV_STORAGE_F64, the state
 * after a setup, releases both.  With F32 every application -- spmvHipFsaiApply, the dM of hipSpCGCSR / hipSpBiCGStabCSR /
 * hipSpGMRESCSR, and the two SpMM passes of the block solvers -- is G~^T (G~ r) with G~_p = (double)(float)G_p: two f32
 * products in serial order (hipSpMVRowsCSRf32 / hipSpMMRowsCSRf32), arithmetic in double.  Rounding is elementwise, so
 * G~^T is the transpose of G~ and M^-1 stays symmetric positive semi-definite; the solution's accuracy is the outer
 * loop's.  spmvHipFsaiRefresh keeps the setting: the forms follow the new values.  Back to F64 gives the f64 bits again.
 * G itself keeps its double values: the f64 launchers on dG are unchanged by the setting.  Synchronous, allocates 4 B per
 * entry of G and of G^T; idempotent.  Refused with a message, the setting left as it was: what spmvHipFsaiInfo refuses, a
 * storage that is neither constant; a failed allocation leaves the factor in F64 with no form.
 * spmvHipFsaiStorage reads the setting back. */
#define SPMV_STORAGE_F64 0
#define SPMV_STORAGE_F32 1
int spmvHipFsaiSetStorage(spmat* dG, int storage);
int spmvHipFsaiStorage(spmat* dG, int* storage);
/* ------------------------------------------------------------- Krylov solves */
/* spmvHipDot: *dResult (one double on the device) = u . v over n elements, in an order that is a function of n alone --
 * not of the grid, the device, the stream, the alignment of the pointers or the run.  DESIGN.md section 19.  Every
 * product u[i] * v[i] is rounded on its own (no FMA), then:
 *     blocks of 4096 consecutive indices, block c = [4096 c, 4096 c + 4096), the last one padded with +0.0 products;
 *     in block c, 256 lane partials from +0.0: lane t adds the products of indices 4096 c + 512 s + 2 t and
 *         4096 c + 512 s + 2 t + 1 for s = 0, 1, ..., 7, in that (ascending) order;
 *     the 256 lane partials a[0..255] meet in the tree: for h = 128, 64, 32, ..., 1: a[t] = a[t] + a[t + h], t < h;
 *         the block partial is a[0];
 *     the block partials P[0..nb-1] by the same rule: lane t adds P[t], P[t + 256], ... in order from +0.0, then the
 *         same tree; the result is a[0].
 *   n = 0 gives +0.0.  Pointers that are only 8-byte aligned give the same bits.  Kernels only, on the library stream: the
 *   block partials go to a library workspace that grows (allocation, device synchronisation) at the first call with more
 *   than any earlier n; calls up to that n only enqueue and can be captured into a graph.  Calls on different streams
 *   share the workspace: keep them ordered.  spmvHipSetSync(1) waits and sets spmvHipLastKernelSeconds; spmvHipSetSync(0)
 *   only enqueues.  spmvHipFinalize frees the workspace.  Refused (EXIT_FAILURE): a NULL dResult, a NULL dU or dV
 *   when n > 0.
 *
 * hipSpCGCSR (A symmetric positive definite) and hipSpBiCGStabCSR (A square, right-preconditioned) solve A x = b on the
 * device.  dX holds x0 on entry and x on return; dM NULL means no preconditioner, otherwise M^-1 v is
 * hipSpTRSVCSR(dM, UPPER, STORED, hipSpTRSVCSR(dM, LOWER, UNIT, v)) -- the ILU(0) pair of hipSpILU0CSR; dM == dA is
 * allowed.  A dM made by spmvHipAmgSetup(dA) (hipSpGMRESCSR too) makes M^-1 v = V(0, v), the cycle of spmvHipAmgApply: its
 * kernels stop with the loop as the triangular solves do, its SpMVs run regardless, info.launches counts them all; a
 * hierarchy of another source is refused.  A dM made by spmvHipFsaiSetup (all three, and the block solvers) makes
 * M^-1 v = G^T (G v), the two serial-order SpMVs of spmvHipFsaiApply through the handle's workspace (a block solve: two SpMM
 * passes through one more block of its own workspace): they run regardless of the stop flag and count as two launches; the
 * factor need not come from this dA -- a lagged preconditioner is legitimate -- but must have dA's size.  x, info.status, info.iterations, info.rr and history are the bits of these loops, in IEEE double with no FMA:
 * dot() is spmvHipDot, A v is serial-order SpMV (sgemvSerial's bits, spmvHipEnqueueAutoRows: its first call for a handle
 * chooses the kernel), every a + s*v is two roundings in the order written, tol2 = tol*tol is computed on the host.
 *     q = A x; r = b - q; rr = dot(r,r); bb = dot(b,b); thresh = tol2 * bb; hist[0] = rr
 *     if rr <= thresh: CONVERGED, 0;  if rr is not finite: NONFINITE, 0;  if maxIter == 0: MAXITER, 0
 *   CG                                            BiCGStab
 *     z = M^-1 r (z = r without M)                  rhat = r; rho = rr; rho_old = alpha = omega = 1
 *     rz = dot(r,z) (rz = rr without M); p = z      if rho == 0: BREAKDOWN, 0
 *     for k = 1 .. maxIter:                         for k = 1 .. maxIter:
 *       q = A p; pq = dot(p,q)                        p = k == 1 ? r : r + beta*(p - omega*v)
 *       if pq == 0: BREAKDOWN, k-1                    phat = M^-1 p (phat = p without M); v = A phat; rv = dot(rhat,v)
 *       alpha = rz / pq                               if rv == 0: BREAKDOWN, k-1
 *       x = x + alpha*p; r = r - alpha*q              alpha = rho / rv; s = r - alpha*v; rr = dot(s,s); hist[k] = rr
 *       rr = dot(r,r); hist[k] = rr                   if rr <= thresh: x = x + alpha*phat; CONVERGED, k
 *       if rr <= thresh: CONVERGED, k                 shat = M^-1 s (shat = s without M); t = A shat
 *       if rr is not finite: NONFINITE, k             tt = dot(t,t); ts = dot(t,s)
 *       if k == maxIter: MAXITER, k                   if tt == 0: x = x + alpha*phat; BREAKDOWN, k
 *       z = M^-1 r; rzn = dot(r,z)                    omega = ts / tt
 *         (without M: z = r, rzn = rr)                x = (x + alpha*phat) + omega*shat; r = s - omega*t
 *       beta = rzn / rz; rz = rzn                     rr = dot(r,r); hist[k] = rr; rhon = dot(rhat,r)
 *       p = z + beta*p                                if rr <= thresh: CONVERGED, k
 *                                                     if rr is not finite: NONFINITE, k
 *                                                     if omega == 0: BREAKDOWN, k
 *                                                     if k == maxIter: MAXITER, k
 *                                                     rho_old = rho; rho = rhon; if rho == 0: BREAKDOWN, k
 *                                                     beta = (rho / rho_old) * (alpha / omega)
 *   "STATUS, j" ends the loop with info.status = STATUS and info.iterations = j.  info.rr is the last rr the loop set
 *   (BiCGStab: dot(s,s) at a half-step exit), info.bb = bb; opts.history (NULL, or room for maxIter + 1 host doubles)
 *   receives hist[0 .. iterations]; later entries are not written.
 * Execution: the scalars and the status live in a device state block that the dot finish kernels write; every kernel
 *   that writes x, r, p or the state, and every triangular solve of M, returns at once once the loop has stopped.  The host
 *   enqueues K iterations, then reads the state back once (info.hostChecks); iterations past the stop write nothing.
 *   K = 16 (spmvHipSetVariant("hipSpCGCSR" / "hipSpBiCGStabCSR", K), 1 <= K <= 4096); x does not change by a bit.
 *   info.launches counts the kernels enqueued (an SpMV counted as one), info.ms the host wall time of the call.
 *   Workspace (CG 3 vectors, 4 with M; BiCGStab 6, 8 with M; 16 B per 4096 rows; history) is allocated by the call and
 *   freed before it returns; the triangles of dM are analysed by the call when they are not yet.  Synchronous, on the
 *   library stream; not capturable.  M = 0 succeeds: CONVERGED, 0, no kernel and no read-back; history[0] = +0.0
 *   (dot(r,r) over no elements) is all it writes.
 * Returns EXIT_SUCCESS whatever the status (info may be NULL).  Refused with a message and EXIT_FAILURE, x untouched:
 *   NULL dA, dB, dX or opts, or a handle that is not live; ELL handles; M != N; dM of another size; dB and dX overlapping; tol negative or
 *   NaN; a history with maxIter + 1 overflowing; for dM the limits of hipSpTRSVCSR and a row without exactly one diagonal
 *   entry (STORED). */
#define SPMV_KRYLOV_CONVERGED 0
#define SPMV_KRYLOV_MAXITER   1
#define SPMV_KRYLOV_BREAKDOWN 2
#define SPMV_KRYLOV_NONFINITE 3
typedef struct {
    double  tol;            /* stop when dot(r,r) <= (tol*tol) * dot(b,b)                  */
    ulong   maxIter;        /* iterations at most                                           */
    double* history;        /* NULL, or maxIter + 1 host doubles: hist[0 .. iterations]      */
} spmvKrylovOpts;
typedef struct {
    int    status;          /* SPMV_KRYLOV_*                                                 */
    ulong  iterations;
    double rr;              /* the last squared residual the loop computed                   */
    double bb;              /* dot(b,b)                                                      */
    ulong  launches;        /* kernels enqueued (an SpMV counted as one)                     */
    ulong  hostChecks;      /* read-backs of the device state                                */
    double ms;              /* host wall time of the call                                    */
} spmvKrylovInfo;
int spmvHipDot(size_t n, const double* dU, const double* dV, double* dResult);
int hipSpCGCSR(spmat* dA, spmat* dM, const double* dB, double* dX, const spmvKrylovOpts* opts, spmvKrylovInfo* info);
int hipSpBiCGStabCSR(spmat* dA, spmat* dM, const double* dB, double* dX, const spmvKrylovOpts* opts, spmvKrylovInfo* info);
/* Blocks of right-hand sides.  DESIGN.md section 27.
 *
 * spmvHipBlockDot: dH[c] (k doubles on the device) = U(:, c) . V(:, c) for c = 0 .. k-1 in one pass.  U and V are n x k on
 * the device, each in its own layout with its own leading dimension, exactly those of hipSpMMRowsCSR:
 * SPMV_DENSE_ROW_MAJOR (element (i, c) at P[i*ld + c], ld >= k) or SPMV_DENSE_COL_MAJOR (P[c*ld + i], ld >= n).  Every
 * dH[c] is bit for bit spmvHipDot(n, U(:, c), V(:, c)): the same blocks of 4096 indices, the same lane order (indices
 * 512 s + 2 t and 512 s + 2 t + 1, s ascending), the same 256-lane tree and the same second level -- whatever k, the
 * layouts, the leading dimensions and the alignment of the pointers are (16-byte accesses are used where a block allows
 * them: row-major, even leading dimension, even k, 16-byte aligned; the bits do not depend on it).  U == V is allowed;
 * n = 0 gives k times +0.0.  Kernels only, on the library stream; the block partials go to the library's dot workspace
 * (here (k rounded up to even) * ceil(n / 4096) doubles), so a call can be captured once the workspace is large enough, as
 * spmvHipDot.  spmvHipSetSync as for spmvHipDot.  Refused (EXIT_FAILURE): a NULL dH, a NULL dU or dV when n > 0, k = 0, an
 * unknown layout, a leading dimension too small for its layout.
 *
 * hipSpCGBlockCSR / hipSpBiCGStabBlockCSR: k independent solves A x_c = b_c advanced in lock step -- not a block Krylov
 * method: no Krylov space is shared.  B and X are M x k on the device, each in its own layout and leading dimension (the
 * rules of hipSpTRSMCSR); X holds X0 on entry.  One opts.tol and one opts.maxIter apply to every column; the threshold is
 * the column's own, tol2 * dot(b_c, b_c).  cols is NULL or k host records; opts.history is NULL or k * (maxIter + 1) host
 * doubles, column c's history at history + c * (maxIter + 1), of which only hist[0 .. iterations_c] is written.
 *   Bits: for every column c, X(:, c), cols[c].status, .iterations, .rr, .bb and the column's history are the bits of
 *   hipSpCGCSR / hipSpBiCGStabCSR on (dA, dM, B(:, c), X0(:, c)) -- the loops written out above.  A column that has
 *   stopped is frozen: its x is the loop's x however many more iterations its neighbours run and however far a batch of K
 *   iterations overshoots; BiCGStab's half-step write x = x + alpha*phat is made per column.  Columns are independent: a
 *   NaN, an Inf or a breakdown in one never reaches another.  Elements of X outside the M x k block are never written; B
 *   is only read.
 *   info: status is the largest column status, iterations the largest column count, rr and bb those of the
 *   lowest-numbered column that has info.status; launches, hostChecks and ms as in the single solves.  info.launches does
 *   not depend on k: an iteration is one hipSpMMRowsCSR pass (counted as one, also for k > 16), the two hipSpTRSMCSR
 *   passes of dM, and one launch per fused pass and per scalar step, each covering all columns.
 *   dM: NULL, or an ILU(0) handle, applied as hipSpTRSMCSR(LOWER, UNIT) then (UPPER, STORED); dM == dA is allowed.  Or a
 *   multigrid hierarchy of dA that was given a block workspace of width >= k (spmvHipAmgSetBlockWidth below): M^-1 is one
 *   block cycle (spmvHipAmgApplyBlock) for all columns, every launch of it behind the same stop word, and it adds that
 *   cycle's launch count, which does not depend on k either, to info.launches; the cycle's Z is scratch and a stopped
 *   column's Z is never read.  Column c then has the bits of the single solve with (dA, dM).  A hierarchy without a
 *   workspace, with width < k, or with a Gauss-Seidel level is refused (the line contains "multigrid hierarchy").
 *   Execution: one state block per column on the device; one finish launch runs every column's scalar step; every kernel
 *   that writes x, r, p, s or a column's state leaves a stopped column alone.  A word that is set when the last column
 *   stops is what the host reads once per K iterations (spmvHipSetVariant("hipSpCGBlockCSR" / "hipSpBiCGStabBlockCSR", K),
 *   1 <= K <= 4096, default 16) and what the triangular passes take as their stop pointer; it is also read once after the
 *   init, so a block whose columns all stop there enqueues no further kernel.  Workspace (the vectors of the single solve
 *   times k rounded up to even, the partials, the states, the history) is allocated by the call and freed before it
 *   returns.  Synchronous, on the library stream; not capturable.  M = 0 succeeds: every column CONVERGED, 0, no kernel;
 *   history + c * (maxIter + 1) receives +0.0.  (k = 1 with unit strides runs the single solve, at the block's K.)
 * Returns EXIT_SUCCESS whatever the statuses (cols and info may be NULL).  Refused with a message and EXIT_FAILURE, X
 *   untouched: what the single solves refuse; k = 0, an unknown layout, a leading dimension too small for its layout, any
 *   overlap of the address spans of B and X (the checks of hipSpTRSMCSR); a history of k * (maxIter + 1) doubles
 *   overflowing; a multigrid hierarchy as dM that cannot run a block cycle of k columns (checked first of all, after k = 0). */
typedef struct {
    int    status;          /* SPMV_KRYLOV_* of this column                                  */
    ulong  iterations;
    double rr;              /* the last squared residual the column's loop computed          */
    double bb;              /* dot(b_c, b_c)                                                 */
} spmvKrylovColumn;
int spmvHipBlockDot(size_t n, unsigned k, const double* dU, size_t ldu, int uLayout, const double* dV, size_t ldv, int vLayout,
                    double* dH);
int hipSpCGBlockCSR(spmat* dA, spmat* dM, unsigned k, const double* dB, size_t ldb, int bLayout, double* dX, size_t ldx,
                    int xLayout, const spmvKrylovOpts* opts, spmvKrylovColumn* cols, spmvKrylovInfo* info);
int hipSpBiCGStabBlockCSR(spmat* dA, spmat* dM, unsigned k, const double* dB, size_t ldb, int bLayout, double* dX, size_t ldx,
                          int xLayout, const spmvKrylovOpts* opts, spmvKrylovColumn* cols, spmvKrylovInfo* info);
/* spmvHipMultiDot: dH[i] (k doubles on the device) = V(:, i) . w for i = 0 .. k-1 in one pass over w, column i of V at
 * dV + i*ldv (ldv >= n).  Every dH[i] is bit for bit spmvHipDot(n, dV + i*ldv, dW): the same blocks of 4096 indices, the
 * same lane order, the same tree and the same second level -- whatever k, ldv and the alignment of the pointers are
 * (one form is chosen per call on the host: 16-byte loads when dV and dW are 16-byte aligned and, for k > 1, ldv is even;
 * scalar loads otherwise).  DESIGN.md section 20.  Two kernels on the library stream: the first keeps a block's 16 doubles
 * of w per lane in registers and walks the columns (panels of 16 in the grid's z), block partials to part[i*nb + blk];
 * the second adds them, one workgroup per pair of columns.  No flags, tickets or atomics: the kernel boundary orders them.
 *   n = 0 writes k times +0.0.  dH[k ..] is not touched.
 *   Workspace: the library's dot workspace, shared with spmvHipDot, here k * ceil(n / 4096) doubles: it grows (allocation,
 *   device synchronisation) at the first call that needs more than any earlier call of either function; calls within
 *   that size only enqueue and can be captured into a graph.  Calls on different streams share it: keep them ordered.
 *   spmvHipSetSync, spmvHipLastKernelSeconds and spmvHipLastLaunch as for spmvHipDot (the last launch is the second
 *   kernel: ceil(k/2) workgroups of 256).  spmvHipFinalize frees the workspace.
 *   Refused (EXIT_FAILURE, dH untouched): a NULL dH; a NULL dV or dW when n > 0; k == 0; ldv < n.
 *
 * hipSpGMRESCSR: right-preconditioned restarted GMRES(restart) for a square A, with classical Gram-Schmidt applied twice
 * (CGS2).  dA, dM, dB, dX, info as for the two solvers above; opts.restart in 1 .. 64; opts.maxIter counts inner
 * iterations (Arnoldi steps) over all cycles.  x, info.status, info.iterations, info.rr, info.bb and history are the bits
 * of this loop, in IEEE double with no FMA: dot() is spmvHipDot, A v is serial-order SpMV, M^-1 the two hipSpTRSVCSR
 * solves, sqrt and / are correctly rounded, every a +- s*v is two roundings in the order written, tol2 = tol*tol on the
 * host.  v[0 .. restart], w, z, u, r, q are vectors; h, c, cs, sn, g, y and the upper triangle R are scalars.
 *     q = A x; r = b - q; rr = dot(r,r); bb = dot(b,b); thresh = tol2 * bb; hist[0] = rr
 *     if rr <= thresh: CONVERGED, 0;  if rr is not finite: NONFINITE, 0;  if maxIter == 0: MAXITER, 0
 *     k = 0
 *     cycle:
 *       beta = sqrt(rr); v[0] = r / beta (element by element); g[0] = beta
 *       for j = 0 .. restart-1:
 *         z = M^-1 v[j] (z = v[j] without M); w = A z
 *         for i = 0..j: h[i] = dot(v[i], w)                            -- spmvHipMultiDot
 *         for i = 0..j ascending: w = w - h[i]*v[i]
 *         for i = 0..j: c[i] = dot(v[i], w)                            -- the second pass
 *         for i = 0..j ascending: w = w - c[i]*v[i]
 *         for i = 0..j: h[i] = h[i] + c[i]
 *         ww = dot(w,w); hn = sqrt(ww)
 *         for i = 0..j-1: t = cs[i]*h[i] + sn[i]*h[i+1]; h[i+1] = cs[i]*h[i+1] - sn[i]*h[i]; h[i] = t
 *         d = sqrt(h[j]*h[j] + hn*hn)
 *         if d == 0:                                                   -- the step is dropped: k and hist are as before it
 *           if j == 0: BREAKDOWN, k                                    -- nothing to add to x; rr, hist[k] stay the last true ones
 *           cols = j; go to endcycle
 *         k = k + 1
 *         cs[j] = h[j]/d; sn[j] = hn/d; h[j] = d; R[0..j][j] = h[0..j]
 *         g[j+1] = -(sn[j]*g[j]); g[j] = cs[j]*g[j]; est = g[j+1]*g[j+1]; hist[k] = est
 *         if est <= thresh or est is not finite or hn == 0 or j == restart-1 or k == maxIter: cols = j+1; go to endcycle
 *         v[j+1] = w / hn
 *       endcycle (cols >= 1):
 *         for i = cols-1 .. 0: s = g[i]; for l = i+1 .. cols-1 ascending: s = s - R[i][l]*y[l]; y[i] = s / R[i][i]
 *         u = y[0]*v[0]; for i = 1 .. cols-1: u = u + y[i]*v[i];  z = M^-1 u (z = u without M);  x = x + z
 *         q = A x; r = b - q; rr = dot(r,r); hist[k] = rr              -- the TRUE residual replaces the estimate
 *         if rr <= thresh: CONVERGED, k;  if rr is not finite: NONFINITE, k
 *         if the cycle ended on hn == 0 or d == 0: BREAKDOWN, k
 *         if k == maxIter: MAXITER, k;  else the next cycle
 *   CONVERGED is only ever declared on the true dot(b - A x, b - A x), never on the estimate.  hist[k] is the estimate
 *   inside a cycle and the true rr at index 0 and at every cycle's last index; info.rr is the last true rr.
 *   The corners: a step with d == 0 does not count (k is the number of steps before it) and writes no hist entry; at
 *   j == 0 the solve ends there with x, info.rr and hist[k] as the previous cycle end (or the init) left them; at j > 0 the
 *   cycle ends with the j columns it has, hist[k] (the last kept step's estimate) becomes the true rr, and the status is
 *   BREAKDOWN unless that rr converged or is not finite.
 * Execution: the scalars live in a device state block that only single-lane finish steps write; the Givens step, the
 *   tests and, at a cycle's end, the back-substitution run on one lane of the ww finish.  The block carries `stop` and,
 *   next to it, `skip` (set when a cycle ends, cleared by the cycle-end step that starts the next one; stop implies
 *   skip): the kernels of an inner step and its triangular solves return at once on skip, those of the cycle end on stop.
 *   The host enqueues one whole cycle -- min(restart, maxIter - k) inner steps, then the cycle end -- and reads the block
 *   back once per cycle: info.hostChecks is the number of cycles (the one read after the init step, which decides
 *   whether a first cycle runs at all, is not counted); steps enqueued past an early cycle end write nothing.  Per inner
 *   step: M^-1, the SpMV, and 8 launches whatever j is (two for each projection, the two updates -- w read and written
 *   once, the v[i] streamed; the second carries the partials of dot(w,w) --, the ww finish, v[j+1] = w / hn);
 *   spmvHipSetVariant("hipSpGMRESCSR", 1) folds the first update into the partials of the second projection (7; the bits
 *   do not change), 0 is the default.
 *   Workspace, allocated by the call and freed before it returns, with ldv = n rounded up to even and nb = ceil(n/4096):
 *   8*ldv*(restart + 4) bytes (v[0 .. restart], w / u, r, q), 8*ldv more with M (z), 8*nb*(restart + 2) of partials,
 *   about 36 KiB of state, 8*(maxIter + 1) with a history.  Synchronous, on the library stream; not capturable.
 *   M = 0 succeeds as above: CONVERGED, 0, history[0] = +0.0, no kernel and no read-back.
 * Refused with a message and EXIT_FAILURE, x untouched: everything hipSpBiCGStabCSR refuses; restart == 0 or > 64. */
typedef struct {
    double   tol;           /* stop when the true dot(r,r) <= (tol*tol) * dot(b,b)            */
    ulong    maxIter;       /* inner iterations at most, over all cycles                     */
    unsigned restart;       /* inner iterations of a cycle, 1 .. 64                          */
    double*  history;       /* NULL, or maxIter + 1 host doubles: hist[0 .. iterations]      */
} spmvGmresOpts;
int spmvHipMultiDot(size_t n, unsigned k, const double* dV, size_t ldv, const double* dW, double* dH);
int hipSpGMRESCSR(spmat* dA, spmat* dM, const double* dB, double* dX, const spmvGmresOpts* opts, spmvKrylovInfo* info);
/* ------------------------------------------------------------- basis rotation, extreme eigenpairs */
/* spmvHipBlockCombine: Y = V S on the device, next to spmvHipMultiDot: V is n x m, S is m x k, Y is n x k, all
 * column-major (V(i, j) at dV[j*ldv + i], ldv >= n; S[j][c] at dS[c*lds + j], lds >= m; Y(i, c) at dY[c*ldy + i], ldy >= n),
 * 1 <= m <= 64, 1 <= k <= 64.
 *     Y(i, c) = +0.0;  for j = 0 .. m-1 ascending:  Y(i, c) = Y(i, c) + V(i, j) * S[j][c]
 * in IEEE double, every product and every add rounded on its own (no FMA, no matrix instruction) -- whatever n, the
 * leading dimensions and the alignment of the pointers are (one form is chosen per call on the host: a lane owns two
 * adjacent rows with 16-byte accesses when m <= 32, dV and dY are 16-byte aligned, ldv is even or m == 1, and ldy is even
 * or k == 1; one row with 8-byte accesses otherwise).  A row's m values are all read before any of its k sums is stored,
 * and a row touches no other row: dY == dV with ldy == ldv is allowed (in place, k <= m); a NaN or an Inf in one row of V
 * stays in that row.  Rows >= n and columns >= k of Y, and everything of V outside Y, are not written.  n = 0 launches nothing.
 *   One kernel on the library stream, no workspace: capturable.  spmvHipSetSync, spmvHipLastKernelSeconds and
 *   spmvHipLastLaunch as for spmvHipDot.  It streams 8*n*(m + k) bytes.
 *   Refused (EXIT_FAILURE, dY untouched): a NULL dV, dS or dY when n > 0; m or k outside 1 .. 64; ldv < n, ldy < n,
 *   lds < m; dY == dV with k > m or ldy != ldv; any other overlap of the spans of dV and dY, or of dS and dY.
 *
 * hipSpLanczosCSR: the nev algebraically largest (SPMV_EIG_LARGEST) or smallest (SPMV_EIG_SMALLEST) eigenpairs of a
 * symmetric square CSR handle by thick-restart Lanczos with full reorthogonalisation (classical Gram-Schmidt applied
 * twice).  Symmetry of A is the caller's promise, as it is for hipSpCGCSR: nothing checks it.  theta, res, X, info.status,
 * .found, .iterations, .cycles, .hostChecks, .scale and .sweepsMax are the bits of this loop, in IEEE double with no FMA:
 * dot() is spmvHipDot, A v is serial-order SpMV, sqrt and / are correctly rounded, every a +- s*v is two roundings in the
 * order written.  m = opts.ncv; v[0 .. m], w are vectors; T is m x m, symmetric, on the host.
 *     nn = dot(v0,v0)
 *     if nn is not finite: NONFINITE, 0 found;  if nn == 0: BREAKDOWN, 0 found;  if maxIter == 0: MAXITER, 0 found
 *     v[0] = v0 / sqrt(nn) (element by element);  k = 0;  T = 0;  it = 0;  cycles = 0
 *     kk = opts.keep, or for keep == 0: min(m-1, nev + (m - nev)/2) (integer division)
 *     cycle:  cycles = cycles + 1
 *       for j = k .. m-1:
 *         w = A v[j];  it = it + 1
 *         for i = 0..j: h[i] = dot(v[i], w)                            -- spmvHipMultiDot
 *         for i = 0..j ascending: w = w - h[i]*v[i]
 *         for i = 0..j: c[i] = dot(v[i], w)                            -- the second pass
 *         for i = 0..j ascending: w = w - c[i]*v[i]
 *         alpha = h[j] + c[j];  T[j][j] = alpha;  beta = sqrt(dot(w,w))
 *         if alpha or beta is not finite: NONFINITE, 0 found
 *         if beta == 0: cols = j+1; exact = true; go to ritz           -- an invariant subspace
 *         v[j+1] = w / beta;  if j+1 < m: T[j][j+1] = T[j+1][j] = beta
 *         if it == maxIter: cols = j+1; go to ritz
 *       cols = m
 *     ritz:
 *       (d, S) = JACOBI(T[0..cols-1][0..cols-1]);  if it did not end, or a d[i] is not finite: NONFINITE, 0 found
 *       order the columns: d ascending (SMALLEST) or descending (LARGEST), equal values by ascending index: theta, S
 *       res[i] = exact ? +0.0 : |beta * S[cols-1][i]|;  scale = max over all cols of |theta[i]|
 *       found = min(nev, cols);  done = cols >= nev and res[i] <= tol*scale for every i < nev
 *       if done or exact or it == maxIter:
 *         X(:, i) = sum over j = 0..cols-1 of v[j] * S[j][i] for i < found              -- spmvHipBlockCombine
 *         CONVERGED if done;  else BREAKDOWN if exact (res is +0.0 then, so `done` fails only on cols < nev: BREAKDOWN
 *         means that the Krylov space of v0 holds fewer than nev pairs, and found = cols of them are returned);  else MAXITER
 *       V(:, i) = sum over j = 0..m-1 of v[j] * S[j][i] for i < kk (in place);  v[kk] = v[m]
 *       T = 0;  T[i][i] = theta[i], T[kk][i] = T[i][kk] = beta * S[m-1][i] for i < kk;  k = kk;  next cycle
 *   JACOBI(T), n = cols: A = T, S = I; sweeps of the pairs p < q by rows (p = 0..n-2, q = p+1..n-1); for a pair with
 *   a = A[p][q]: if a == 0 nothing; if |A[p][p]| + |a| == |A[p][p]| and |A[q][q]| + |a| == |A[q][q]| then A[p][q] = A[q][p] = 0
 *   and no rotation; else th = (A[q][q] - A[p][p]) / (2*a); t = 1 / (|th| + sqrt(th*th + 1)), negated when th < 0;
 *   c = 1 / sqrt(t*t + 1); s = t*c; tau = s / (1 + c); for r other than p, q, with x = A[r][p], y = A[r][q]:
 *   A[r][p] = A[p][r] = x - s*(y + tau*x), A[r][q] = A[q][r] = y + s*(x - tau*y); A[p][p] -= t*a, A[q][q] += t*a,
 *   A[p][q] = A[q][p] = 0; for every r, with x = S[r][p], y = S[r][q]: S[r][p] = x - s*(y + tau*x), S[r][q] = y + s*(x - tau*y).
 *   It ends after the first sweep without a rotation (d = the diagonal of A); 30 sweeps that all rotated do not end.
 *   info.sweepsMax is the most sweeps any cycle took (the last, rotation-free one included).
 * Outputs: dX is n x nev on the device, column-major with ldx >= n; theta and res are nev host doubles each.  Only the
 *   first info.found columns and entries are written.  dV0 (n doubles) is only read and must not overlap dX; the library
 *   supplies no start vector.  info.iterations counts the products A v, opts.maxIter caps them over all cycles.
 * Execution: one device state block with `stop` and `skip`, as in hipSpGMRESCSR: a step with beta == 0, the step that
 *   reaches maxIter and a step with a value that is not finite set skip, and the cycle's remaining enqueued kernels
 *   return at once.  The host enqueues the m - k steps of a cycle (fewer when maxIter is nearer), reads alpha[], beta[]
 *   and the flags back once (info.hostChecks: the number of cycles; the read after v[0] is not counted), runs JACOBI on
 *   the host inside that wait, uploads the cols x kk (or cols x found) block of S and enqueues the rotation.  Per step:
 *   the SpMV and 8 launches whatever j is (two for each projection, the two updates -- the second carries the partials
 *   of dot(w,w) --, the scalar step, v[j+1] = w / beta); per cycle one rotation more; 3 launches before the first cycle.
 *   info.launches counts them (the uploads of S and the copy v[kk] = v[m] are copies, not launches); info.ms is the
 *   host wall time of the call and info.jacobiMs the part of it spent in JACOBI.
 *   Workspace, allocated by the call and freed before it returns, with ldv = n rounded up to even and nb = ceil(n/4096):
 *   8*ldv*(ncv + 2) bytes (v[0 .. ncv], w), 8*nb*(ncv + 1) of partials, 32 KiB for S, about 2 KiB of state.
 *   Synchronous, on the library stream; not capturable.
 * Returns EXIT_SUCCESS whatever the status (info may be NULL).  Refused with a message and EXIT_FAILURE, every output
 *   untouched: NULL dA, dV0, opts, dX, theta or res, or a handle that is not live; ELL handles; M != N; nev == 0,
 *   nev >= ncv, ncv > 64 or ncv > M; an unknown which; tol negative or NaN; keep not 0 and outside nev .. ncv-1;
 *   ldx < M; dV0 overlapping the span of dX. */
#define SPMV_EIG_LARGEST  0
#define SPMV_EIG_SMALLEST 1
typedef struct {
    unsigned nev;           /* eigenpairs wanted, 1 .. ncv-1                                 */
    unsigned ncv;           /* m: Lanczos vectors of a cycle, nev+1 .. min(64, M)            */
    int      which;         /* SPMV_EIG_LARGEST or SPMV_EIG_SMALLEST (algebraically)         */
    double   tol;           /* converged when res[i] <= tol * scale for every i < nev        */
    ulong    maxIter;       /* products A v at most, over all cycles                         */
    unsigned keep;          /* columns a restart keeps, nev .. ncv-1; 0: the default         */
} spmvLanczosOpts;
typedef struct {
    int      status;        /* SPMV_KRYLOV_*                                                 */
    unsigned found;         /* eigenpairs written                                            */
    ulong    iterations;    /* products A v                                                  */
    ulong    cycles;
    ulong    launches;      /* kernels enqueued (an SpMV counted as one)                     */
    ulong    hostChecks;    /* read-backs of the device state: the cycles                    */
    double   scale;         /* max |theta[i]| over the last cycle's Ritz values              */
    unsigned sweepsMax;     /* the most Jacobi sweeps a cycle took                           */
    double   ms;            /* host wall time of the call                                    */
    double   jacobiMs;      /* of which inside JACOBI, over all cycles                       */
} spmvLanczosInfo;
int spmvHipBlockCombine(size_t n, unsigned m, unsigned k, const double* dV, size_t ldv, const double* dS, size_t lds, double* dY,
                        size_t ldy);
int hipSpLanczosCSR(spmat* dA, const double* dV0, const spmvLanczosOpts* opts, double* dX, size_t ldx, double* theta, double* res,
                    spmvLanczosInfo* info);
/* ------------------------------------------------------------- residual block, preconditioned eigensolver */
/* spmvHipBlockResidual: R = W S - (V S) diag(theta) and the squared norms of R's columns in one pass, next to
 * spmvHipBlockCombine and with its conventions: V and W are n x m, S is m x k, R is n x k, all column-major (V(i, j) at
 * dV[j*ldv + i], W(i, j) at dW[j*ldw + i], S[j][c] at dS[c*lds + j], R(i, c) at dR[c*ldr + i]), theta and norm2 are k device
 * doubles; 1 <= m <= 64, 1 <= k <= 16.  For row i and column c:
 *     u = +0.0;  for j = 0 .. m-1 ascending:  u = u + V(i, j) * S[j][c]          (the bits of spmvHipBlockCombine(V, S))
 *     q = +0.0;  for j = 0 .. m-1 ascending:  q = q + W(i, j) * S[j][c]          (the bits of spmvHipBlockCombine(W, S))
 *     R(i, c) = q - theta[c] * u                                (the product rounded, then the subtraction)
 *     dNorm2[c] = spmvHipDot(R(:, c), R(:, c))                  (its bits: the dot's blocks, lanes, tree and finish)
 * in IEEE double, every product and every add rounded on its own (no FMA, no matrix instruction) -- whatever n, the leading
 * dimensions and the alignment of the pointers are (one form is chosen per call on the host: 16-byte accesses of two adjacent
 * rows when dV, dW and dR are 16-byte aligned, ldv and ldw are even or m == 1, and ldr is even or k == 1; 8-byte accesses
 * otherwise).  With V a basis, W = A V and (theta, S) Ritz pairs of V^T W, column c of R is the residual A x - theta x of
 * the Ritz vector x = V S(:, c).  A row touches no other row: a NaN or an Inf in one row of V or W stays in that row of R
 * (it reaches dNorm2).  Rows >= n and columns >= k of R and entries >= k of dNorm2 are not written.  n = 0 launches nothing
 * and writes nothing, dNorm2 included.
 *   Two kernels on the library stream (the pass, which leaves k block partials per block of 4096 rows in the dot workspace,
 *   and the finish of spmvHipMultiDot); the workspace is grown as spmvHipMultiDot grows it, so the call is capturable once a
 *   call of this size has been made.  spmvHipSetSync, spmvHipLastKernelSeconds and spmvHipLastLaunch as for spmvHipDot.
 *   It streams 8*n*(2*m + k) bytes.
 *   Refused (EXIT_FAILURE, dR and dNorm2 untouched): a NULL pointer when n > 0; m outside 1 .. 64, k outside 1 .. 16;
 *   ldv < n, ldw < n, ldr < n, lds < m; any overlap of the span of dR or of dNorm2 with dV, dW, dS or dTheta, or of dR
 *   with dNorm2.  (dV and dW may be the same block.)
 *
 * hipSpDavidsonCSR: the nev algebraically smallest (or, without a dM, largest) eigenpairs of a symmetric square CSR handle
 * by generalised Davidson with single-vector expansion: the basis grows by the preconditioned residual of the first wanted
 * Ritz pair that has not converged, orthogonalised by classical Gram-Schmidt applied twice; the projected matrix H = V^T A V
 * is kept whole on the host and diagonalised by JACOBI (hipSpLanczosCSR's, above); a full basis is restarted with its kk
 * wanted Ritz vectors.  dM is NULL (t = r: the Krylov space of v0, restarted as Lanczos restarts it) or anything the Krylov
 * solvers take as dM -- an ILU(0) handle applied by level sets or by sweeps, an approximate-inverse factor in either
 * storage, a multigrid hierarchy of dA with any smoother and storage --, and goes through their checks.  Symmetry of A and
 * of M^-1 is the caller's promise.  theta, res, X, info.status, .found, .iterations, .restarts, .precondApplies,
 * .hostChecks, .launches, .scale and .sweepsMax are the bits and counts of this loop, in IEEE double with no FMA: dot() is
 * spmvHipDot, A v is serial-order SpMV, M^-1 r is what hipSpCGCSR applies, sqrt and / are correctly rounded, every
 * a +- s*v is two roundings in the order written.  m = opts.ncv; v[0 .. m-1], w[0 .. m-1] and R (n x nev) are on the
 * device; H is m x m, symmetric, on the host.
 *     nn = dot(v0,v0)
 *     if nn is not finite: NONFINITE, 0 found;  if nn == 0: BREAKDOWN, 0 found;  if maxIter == 0: MAXITER, 0 found
 *     v[0] = v0 / sqrt(nn) (element by element);  cols = 0;  it = 0;  restarts = 0;  H = 0
 *     kk = opts.keep, or for keep == 0: min(m-1, nev + (m - nev)/2) (integer division)
 *     step:
 *       j = cols;  w[j] = A v[j];  it = it + 1
 *       for i = 0..j: H[i][j] = H[j][i] = dot(v[i], w[j])              -- spmvHipMultiDot
 *       cols = j+1;  if one of these is not finite: NONFINITE, 0 found
 *       (d, S) = JACOBI(H[0..cols-1][0..cols-1]);  if it did not end, or a d[i] is not finite: NONFINITE, 0 found
 *       order the columns: d ascending (SMALLEST) or descending (LARGEST), equal values by ascending index: theta, S
 *       scale = max over all cols of |theta[i]|;  c = min(nev, cols)
 *       (R, n2) = spmvHipBlockResidual(v[0..cols-1], w[0..cols-1], S[.][0..c-1], theta[0..c-1]);  res[i] = sqrt(n2[i]) for i < c
 *       if a res[i] is not finite: NONFINITE, 0 found
 *       done = cols >= nev and res[i] <= tol*scale for every i < nev
 *       if done or it == maxIter:
 *         X(:, i) = sum over j = 0..cols-1 of v[j] * S[j][i] for i < c               -- spmvHipBlockCombine
 *         found = c;  CONVERGED if done, else MAXITER
 *       l = the first i < c with res[i] > tol*scale;  if there is none (then cols < nev): l = c-1
 *       if cols == m:                                                   -- the restart
 *         V(:, i) = sum over j of v[j] * S[j][i],  W(:, i) = sum over j of w[j] * S[j][i]  for i < kk (both in place, j = 0..m-1)
 *         H = 0;  H[i][i] = theta[i] for i < kk;  cols = kk;  restarts = restarts + 1
 *       t = M^-1 R(:, l) with a dM (precondApplies = precondApplies + 1), else t = R(:, l)
 *       for i = 0..cols-1: h[i] = dot(v[i], t);  for i = 0..cols-1 ascending: t = t - h[i]*v[i]
 *       for i = 0..cols-1: g[i] = dot(v[i], t);  for i = 0..cols-1 ascending: t = t - g[i]*v[i]        -- the second pass
 *       beta = sqrt(dot(t,t));  if beta is not finite: NONFINITE, 0 found
 *       if beta == 0: BREAKDOWN with found = c and the X, theta, res of this step  -- t lies in the basis: nothing to add
 *       v[cols] = t / beta;  next step
 *   res[i] is the computed norm of the residual A x_i - theta_i x_i formed from the kept products, not an estimate.  The
 *   vectors w[j] are products A v[j] only until the first restart: afterwards they are rotated with the basis and never
 *   recomputed, so W drifts from A V by the rounding of the rotations.  On the reference over the converged cases of the
 *   test table and the 12 x 10 x 8 Laplacian the largest |res[i] - ||A x_i - theta_i x_i||| recomputed from X was 3.8e-15,
 *   the largest |X^T X - I| entry 2.3e-15 and the largest |theta[i] - eigenvalue| 2.7e-14.
 *   BREAKDOWN after a restart step returns the first c columns of the rotated basis, which are the X of that step.
 * Outputs: as hipSpLanczosCSR's (dX n x nev column-major with ldx >= n, theta and res nev host doubles, only the first
 *   info.found written; dV0 only read, not overlapping dX).  info.iterations counts the products A v, opts.maxIter caps them.
 * Execution: one device state block with `stop` and `skip`, as in hipSpLanczosCSR.  A step's expansion (M^-1, the two
 *   projections and updates, beta's scalar step -- it sets skip on beta == 0 and stop on a beta that is not finite --,
 *   v[cols] = t / beta), its product and the new column of H are enqueued together and read back once; JACOBI runs on the
 *   host; theta and S[.][0..c-1] are uploaded, the residual block enqueued and its c norms read back: two read-backs a
 *   step (info.hostChecks; the read after v[0] is not counted; a step that ends on beta has one).  info.launches counts:
 *   3 before the first step; 3 per product enqueued (the SpMV, the two kernels of the new column of H; the product after a
 *   beta that is 0 or not finite is enqueued and counted); 2 per residual block; 8 per expansion (two for each projection, the two updates -- the
 *   second carries the partials of dot(t,t) --, beta's step, the division) and what the dM's application enqueues (hipSpCGCSR
 *   counts the same); 2 per restart; 1 for X.  Uploads are copies, not launches.  info.ms is the host wall time of the call and
 *   info.jacobiMs the part of it spent in JACOBI.
 *   Workspace, allocated by the call and freed before it returns, with ldv = n rounded up to even and nb = ceil(n/4096), in
 *   this order: 8*ldv*ncv bytes (v), 8*ldv*ncv (w), 8*ldv*nev (R), with a dM 8*ldv (t: no application runs in place; without
 *   one t is R's column itself), 8*nb*(ncv + 1) of partials, 32 896 bytes for theta and S, about 1 KiB of state.
 *   Synchronous, on the library stream; not capturable.
 * Returns EXIT_SUCCESS whatever the status (info may be NULL).  Refused with a message and EXIT_FAILURE, every output
 *   untouched: everything hipSpLanczosCSR refuses; nev > 16; a dM with SPMV_EIG_LARGEST (a positive definite M^-1 damps the
 *   wanted directions: on the 21 x 19 x 17 Laplacian the search then took six times the products it takes without a dM, or
 *   did not end); a dM that hipSpCGCSR refuses for dA. */
typedef struct {
    unsigned nev;           /* eigenpairs wanted, 1 .. min(16, ncv-1)                        */
    unsigned ncv;           /* m: columns of the basis at most, nev+1 .. min(64, M)          */
    int      which;         /* SPMV_EIG_SMALLEST; SPMV_EIG_LARGEST only without a dM         */
    double   tol;           /* converged when res[i] <= tol * scale for every i < nev        */
    ulong    maxIter;       /* products A v at most                                          */
    unsigned keep;          /* columns a restart keeps, nev .. ncv-1; 0: the default         */
} spmvDavidsonOpts;
typedef struct {
    int      status;        /* SPMV_KRYLOV_*                                                 */
    unsigned found;         /* eigenpairs written                                            */
    ulong    iterations;    /* products A v                                                  */
    ulong    restarts;
    ulong    precondApplies;/* applications of M^-1                                          */
    ulong    launches;      /* kernels enqueued (an SpMV counted as one)                     */
    ulong    hostChecks;    /* read-backs of the device state                                */
    double   scale;         /* max |theta[i]| over the last step's Ritz values               */
    unsigned sweepsMax;     /* the most Jacobi sweeps a step took                            */
    double   ms;            /* host wall time of the call                                    */
    double   jacobiMs;      /* of which inside JACOBI, over all steps                        */
} spmvDavidsonInfo;
int spmvHipBlockResidual(size_t n, unsigned m, unsigned k, const double* dV, size_t ldv, const double* dW, size_t ldw, const double* dS,
                         size_t lds, const double* dTheta, double* dR, size_t ldr, double* dNorm2);
int hipSpDavidsonCSR(spmat* dA, spmat* dM, const double* dV0, const spmvDavidsonOpts* opts, double* dX, size_t ldx, double* theta,
                     double* res, spmvDavidsonInfo* info);
/* ------------------------------------------------------------- multi-colour ordering, symmetric permutation */
/* Reordering for fewer level sets: if rows of one colour share no entry and the matrix is permuted so that colours are
 * contiguous, both triangles of B = P A P^T have at most as many level sets as there are colours, and hipSpTRSVCSR /
 * hipSpILU0CSR on B run that many launches.  The caller permutes (A, b), solves with B, and permutes x back; every other
 * contract of this header applies to B's arrays unchanged.  DESIGN.md section 21.
 *
 * spmvHipColourCSR colours the vertices of a square CSR handle.  The result is a function of the PATTERN and the options
 *   alone -- not of the run, the grid or the order in which lanes finish -- and is the output of this loop:
 *       adj(i) = { j != i : row i stores column j, or row j stores column i }     (the pattern of A + A^T: repeats count
 *                                                     once, the diagonal is ignored, rows need not be sorted)
 *       key(i) = 0 for SPMV_COLOUR_NATURAL,  fmix32(i ^ seed) for SPMV_COLOUR_HASH, with the murmur3 finaliser
 *                fmix32(h): h ^= h>>16; h *= 0x85ebca6b; h ^= h>>13; h *= 0xc2b2ae35; h ^= h>>16      (32-bit)
 *       j wins against i:  NATURAL  j < i;   HASH  (key(j), j) > (key(i), i) as pairs
 *       for i in the order in which every vertex comes after all that win against it
 *                (NATURAL: 0, 1, .. M-1;  HASH: descending (key, id)):
 *           colour[i] = the smallest c >= 0 that no j in adj(i) winning against i has as colour[j]
 *   NATURAL is first-fit in row order: red-black on a bipartite stencil, but as many rounds as the longest ascending path.
 *   HASH takes more colours and few rounds.  opts == NULL: NATURAL, seed 0.
 *   dColour[i] = that colour (M words).  dPerm = the rows ordered by (colour, id): dPerm[new] = old (M words), the
 *   argument of spmvHipCsrPermute / spmvHipVecPermute.  Either may be NULL.  Column ids >= M of an adopted array are no
 *   vertices and are skipped.
 *   info: colours (largest colour + 1), rounds (launch rounds until no row was left; the only figure that may differ from
 *   run to run), hostChecks (read-backs of the device state: one per K rounds, K = 16 unless
 *   spmvHipSetVariant("spmvHipColourCSR", K)), maxColourRows (rows of the largest colour), longRows (rows with more than 64
 *   adjacency entries: one wavefront each), symmetric (1: the stored pattern was found symmetric and the transposed
 *   pattern was not built; tried when no row stores more than 64 entries), ms (wall time of the call).
 *   Synchronous on the library stream; allocates, so not capturable; temporaries (the transposed pattern 8 B/nnz + 4 B/row,
 *   row lists 16 B/row, the sorts' workspaces) are freed before it returns.  M = 0 succeeds with colours = 0, nothing written.
 * spmvHipCsrPermute writes into dB a new, independent CSR handle of B = P A P^T for ANY permutation dPerm (dPerm[new] =
 *   old; a caller's RCM as well): with inv[dPerm[r]] = r, row r of B holds the entries of row dPerm[r] of A, each column j
 *   as inv[j].  Order inside a row: ascending new column, STABLE for repeated columns, which keep A's stored order -- so a
 *   sorted, repeat-free A gives a B that hipSpILU0CSR accepts.  Values move as bits (NaN payloads, -0.0).  dB is like a
 *   transpose handle: u32 columns, 4-byte row pointers, its own unit detection, every CSR entry point works on it, freed
 *   with hipFreeSpmat; it keeps a 4 B/nnz source-position map.  The library checks on the device that dPerm is a
 *   permutation of 0..M-1 before anything of dB is made.  Build temporaries (20 B/nnz + 4 B/row + the sort's workspace) are
 *   freed before it returns; synchronous, not capturable.
 * spmvHipPermuteRefresh gathers B's values from dA's current value array through that map, then does what
 *   spmvHipValuesChanged(dB) does.  dB records its source's id and refuses any other source, as spmvHipTransposeRefresh.
 * spmvHipVecPermute: inverse == 0: dOut[r] = dIn[dPerm[r]] (b' = P b); inverse != 0: dOut[dPerm[r]] = dIn[r] (x = P^T x').
 *   Bits are copied.  One kernel on the library stream, no allocation: capturable; honours spmvHipSetSync; any 8-byte
 *   alignment.  An entry of dPerm >= n is skipped (nothing is read or written for it).
 * Refused with a message and EXIT_FAILURE, outputs untouched: NULL pointers (dColour, dPerm of spmvHipColourCSR, opts and
 *   info excepted); a handle that is not live; ELL handles; M != N; M >= 2^31 or NZ >= IRP32_LIMIT; dB == dA; a dPerm
 *   with a value >= M or a repeated value; a source column id >= M; an unknown order; a refresh of a handle that is not a
 *   permutation, or from a handle that is not its source; dIn == dOut or overlapping.
 *   ("Outputs untouched" is the promise for these refusals.  After a failed device allocation -- "refused allocations"
 *   above -- spmvHipColourCSR leaves info unwritten, but dColour and dPerm may have been written in part and hold nothing
 *   to rely on; spmvHipCsrPermute leaves dB unwritten.) */
#define SPMV_COLOUR_NATURAL 0
#define SPMV_COLOUR_HASH    1
typedef struct {
    int      order;         /* SPMV_COLOUR_NATURAL or SPMV_COLOUR_HASH                        */
    uint32_t seed;          /* of the HASH keys                                              */
} spmvColourOpts;
typedef struct {
    ulong  colours;         /* largest colour + 1                                            */
    ulong  rounds;          /* rounds until every row had its colour                         */
    ulong  hostChecks;      /* read-backs of the device state                                */
    ulong  maxColourRows;   /* rows of the largest colour class                              */
    ulong  longRows;        /* rows coloured by a wavefront each                             */
    int    symmetric;       /* 1: stored pattern symmetric, transposed pattern not built     */
    double ms;              /* wall time of the call                                         */
} spmvColourInfo;
int spmvHipColourCSR(spmat* dA, const spmvColourOpts* opts, uint32_t* dColour, uint32_t* dPerm, spmvColourInfo* info);
int spmvHipCsrPermute(spmat* dA, const uint32_t* dPerm, spmat* dB);
int spmvHipPermuteRefresh(spmat* dB, spmat* dA);
int spmvHipVecPermute(size_t n, const uint32_t* dPerm, const double* dIn, double* dOut, int inverse);
/* ------------------------------------------------------------- bandwidth-reducing ordering (reverse Cuthill-McKee) */
/* spmvHipRcmCSR computes, on the device, the reverse Cuthill-McKee permutation of a square CSR handle: the ordering that
 * brings the entries of B = P A P^T near the diagonal, which is what the SpMV kernels' x reads and the level sets of ILU(0)
 * live on.  It feeds spmvHipCsrPermute / spmvHipVecPermute unchanged.  DESIGN.md section 37.
 *   The result is a function of the PATTERN and the options alone, and is, word for word, the output of this loop.
 *   Adjacency, degree and column rules are the colouring's: adj(i) = { j != i : row i stores column j, or row j stores
 *   column i }; repeats count once, the diagonal is ignored, rows need not be sorted, column ids >= M of an adopted array
 *   are no vertices and are skipped; deg(i) = |adj(i)|.
 *       unvisited = all vertices; order = empty list
 *       while unvisited is not empty:
 *           r = the unvisited vertex of smallest (deg, id)
 *           if start == SPMV_RCM_START_PERIPHERAL:
 *               L = BFS level structure of r inside unvisited;  n = 1
 *               while n <= maxPasses:
 *                   v = the vertex of L's last level of smallest (deg, id)
 *                   if v == r: break
 *                   Lv = BFS level structure of v inside unvisited;  n = n + 1
 *                   if depth(Lv) > depth(L): r = v; L = Lv
 *                   else: break
 *           queue = [r]; mark r visited
 *           while queue is not empty:
 *               u = pop front; append u to order
 *               append to the queue, and mark visited, the unvisited j in adj(u) in ascending (deg(j), j)
 *       perm = order reversed as a whole          (forward != 0: order itself, plain Cuthill-McKee)
 *   opts == NULL: PERIPHERAL, reversed; maxPasses = 0 means 8.
 *   dPerm[new] = old, M words: the argument of spmvHipCsrPermute / spmvHipVecPermute.  It may be NULL (only info is wanted).
 *   info: components; levels (of the ordering BFS, summed over the components); startBfs (BFS runs spent finding starts: the
 *   n of the loop, summed); maxFrontier (the largest level of the ordering BFS); longRows (vertices with more than 64
 *   adjacency entries: a wavefront expands each); symmetric (1: every row ascends strictly and the stored pattern is
 *   structurally symmetric, so A's own arrays served as the adjacency; 0: the deduplicated pattern of A + A^T was built,
 *   68 B/nnz while it is built, 8 B/nnz + 8 B/row kept until the call returns); bandwidthBefore / bandwidthAfter (max |i - j|
 *   over the stored entries with both ids < M, in A's numbering and in the new one); launches and hostChecks (kernel
 *   launches and read-backs of the device state: the only two figures that may depend on the variant); ms (wall time).
 *   Levels of at most T vertices whose degrees sum to at most 2048 are expanded, one after the other, inside one launch of
 *   one workgroup, which also holds the loop's state; any other ("wide") level takes a launch over its frontier and a
 *   launch of that workgroup to take the result in.  Read-backs (hostChecks): one per launch of the workgroup -- so one per
 *   run of thin levels and one per wide level, of the start search or of the ordering --, one more per wide level of the
 *   ordering (the size of the next level, which its radix sort needs on the host), and one for the figures of info: two
 *   per wide ordering level where one would do if the host kept consecutive wide levels to itself.
 *   T = 1024 unless spmvHipSetVariant("spmvHipRcmCSR", T); no word of dPerm depends on it.  The components are taken one
 *   after the other by that one workgroup, tens of microseconds each: vertices without a neighbour are placed all at once,
 *   but a graph of many small components is slow here (DESIGN.md section 37 has 20 000 disjoint edges measured).
 *   Synchronous on the library stream; allocates, so not capturable; every temporary (32 B/row, 16 B/row more once a wide
 *   level is sorted, 4 B/nnz, the adjacency above, the sorts' workspaces) is freed before it returns.  M = 0 succeeds with
 *   nothing written to dPerm.
 * Refused with a message and EXIT_FAILURE, outputs untouched: a NULL handle; a handle that is not live; ELL handles; M != N;
 *   M >= 2^31 or NZ >= IRP32_LIMIT; an unknown start.  (After a failed device allocation -- "refused allocations" above --
 *   info is left unwritten and dPerm holds nothing to rely on, as for spmvHipColourCSR.) */
#define SPMV_RCM_START_MIN_DEGREE 0
#define SPMV_RCM_START_PERIPHERAL 1
typedef struct {
    int      start;         /* SPMV_RCM_START_MIN_DEGREE or SPMV_RCM_START_PERIPHERAL         */
    unsigned maxPasses;     /* BFS runs of the start search per component; 0: 8              */
    int      forward;       /* != 0: the order itself (Cuthill-McKee), not reversed          */
} spmvRcmOpts;
typedef struct {
    ulong  components;      /* connected components of the adjacency                         */
    ulong  levels;          /* levels of the ordering BFS, summed over the components        */
    ulong  startBfs;        /* BFS runs spent finding starts                                 */
    ulong  maxFrontier;     /* the largest level of the ordering BFS                         */
    ulong  longRows;        /* vertices expanded by a wavefront each                         */
    int    symmetric;       /* 1: A's own arrays served as the adjacency                     */
    ulong  bandwidthBefore; /* max |i - j| over the stored entries, A's numbering            */
    ulong  bandwidthAfter;  /* ... in the new numbering                                      */
    ulong  launches;        /* kernel launches of the call                                   */
    ulong  hostChecks;      /* read-backs of the device state                                */
    double ms;              /* wall time of the call                                         */
} spmvRcmInfo;
int spmvHipRcmCSR(spmat* dA, const spmvRcmOpts* opts, uint32_t* dPerm, spmvRcmInfo* info);
/* ------------------------------------------------------------- sparse matrix product C = A B */
/* spmvHipSpGEMM writes into dC a new, independent CSR handle of C = A B.  A name is a contract, and the contract is the
 * bits of this serial loop on the two handles' arrays (IRP, JA, AS as stored):
 *       for i in 0 .. A.M-1:
 *           for p in A.IRP[i] .. A.IRP[i+1]-1:                 (A's stored order)
 *               k = A.JA[p]
 *               for q in B.IRP[k] .. B.IRP[k+1]-1:             (B's stored order)
 *                   j = B.JA[q]
 *                   if (i, j) is new: acc[i,j] = +0.0
 *                   acc[i,j] = acc[i,j] + (A.AS[p] * B.AS[q])  (product rounded, then the add: contraction is off)
 *           row i of C = the (j, acc[i,j]) in ascending j
 *   Structural: every (i, j) that some product reaches is stored, even when the sum is 0.0; nothing is dropped or added.
 *   A and B may have unsorted rows and repeated (row, col) pairs: each repeat is one more term, in stored order.  Rows of
 *   C ascend strictly and have no repeats, so hipSpILU0CSR, hipSpTRSVCSR and the serial-order SpMV selection accept C as it
 *   is.  The result is a function of the two handles' arrays alone -- not of the run, the grid, the class a row fell into
 *   or the options -- and two calls give the same bits.  Where a term is NaN, C has a NaN at that place; its payload is not
 *   pinned (hardware and host differ in which operand's payload an add keeps).  Every other value is pinned as bits:
 *   +-Inf, -0.0 inputs and sums that cancel to +0.0 included.
 *   dC is like a transpose or permuted handle: u32 columns, 4-byte row pointers, its own unit detection, row blocks; every
 *   CSR entry point works on it; freed with hipFreeSpmat.  dA == dB is allowed (A^2).  Sources: spMatCpyCSR /
 *   spmvHipAdoptCSR / transpose / permuted / product handles, row pointers of 4 or 8 bytes, unit-value handles included.
 *   opts (NULL, or a field 0: the built-in default; a value above the built-in limit is clamped to it) only LOWER the class
 *   limits: a row's class comes from m = min(products of the row, B.N): m <= waveMaxProducts (512) one wavefront with a
 *   1 024-slot hash table in LDS, m <= groupMaxProducts (6 144) one workgroup with 8 192 slots, above that the sorted path
 *   (one stable radix sort per batch of rows whose products fit sortBudgetBytes: 32 B per product, default 256 MiB, limit
 *   4 GiB; a row above the budget is a batch of its own).
 *   Memory: C itself 12 B per entry + 4 B per row, its row blocks, and 4 B per row for the refresh (the rows by class).
 *   Temporaries, freed before the call returns: 20 B per row for the bound and the lists, then 12 B per row for the counts
 *   and their scan, 16 B per sorted row, and 32 B per product of the largest sorted batch + the sort's workspace.
 *   info: products (sum of the bounds), nnzC, maxRowProducts, maxRowNnz, rowsWave / rowsGroup / rowsSorted (they sum to the
 *   rows with a product), sortBatches, tempBytes (peak of the temporaries), symbolicMs / numericMs / ms (wall times).
 *   Synchronous on the library stream; allocates, so not capturable.  opts and info may be NULL.
 *   A.M = 0, A.N = 0, B.N = 0 and "no products" succeed with an empty C: valid row pointers, NZ = 0, SpMV on it gives +0.0.
 * spmvHipSpGEMMRefresh recomputes C's values from the sources' CURRENT value arrays, C's pattern and addresses kept: the
 *   numeric phase only, on the classes of the build, then what spmvHipValuesChanged(dC) does.  dC records both sources'
 *   ids and refuses any other pair, and the same pair in the other order.  The sources' patterns must be unchanged.
 * Refused with a message and EXIT_FAILURE, dC and info untouched: NULL dA, dB or dC; a handle that is not live; an ELL
 *   handle; A.N != B.M; dC == dA or dC == dB; A.M or B.N >= 2^32 - 1; nnz(C) >= IRP32_LIMIT (2^32 - 65536; found after the
 *   symbolic phase, before anything of dC exists); a column id of A that is >= B.M (an adopted array; checked on the
 *   device); a refresh of a handle that is not a product, or from other sources. */
typedef struct {            /* 0 = the built-in default; a value above the built-in limit is clamped to it */
    ulong waveMaxProducts;  /* rows with at most this many products: one wavefront each            */
    ulong groupMaxProducts; /* ... at most this many: one workgroup each; above: the sorted path   */
    ulong sortBudgetBytes;  /* temporaries of one batch of the sorted path                         */
} spmvSpgemmOpts;
typedef struct {
    ulong products, nnzC, maxRowProducts, maxRowNnz;
    ulong rowsWave, rowsGroup, rowsSorted, sortBatches;
    ulong tempBytes;        /* peak of the build's temporaries */
    double symbolicMs, numericMs, ms;
} spmvSpgemmInfo;
int spmvHipSpGEMM(spmat* dA, spmat* dB, const spmvSpgemmOpts* opts, spmat* dC, spmvSpgemmInfo* info);
int spmvHipSpGEMMRefresh(spmat* dC, spmat* dA, spmat* dB, spmvSpgemmInfo* info);
/* ------------------------------------------------------------- sparse matrix sum C = alpha A + beta B */
/* spmvHipCsrAdd writes into dC a new, independent CSR handle of C = alpha A + beta B (A - sigma I, A + A^T, the smoothed
 * prolongator T - omega D^-1 A T, a product followed by a sum).  The contract is the bits of this serial loop on the two
 * handles' arrays (IRP, JA, AS as stored):
 *       for i in 0 .. M-1:
 *           for p in A.IRP[i] .. A.IRP[i+1]-1:                 (A's stored order)
 *               j = A.JA[p];  if (i, j) is new: acc[i,j] = +0.0
 *               acc[i,j] = acc[i,j] + (alpha * A.AS[p])        (product rounded, then the add: contraction is off)
 *           for q in B.IRP[i] .. B.IRP[i+1]-1:                 (B's stored order, after all of A's row)
 *               j = B.JA[q];  if (i, j) is new: acc[i,j] = +0.0
 *               acc[i,j] = acc[i,j] + (beta * B.AS[q])
 *           row i of C = the (j, acc[i,j]) in ascending j
 *   Structural: every (i, j) that A or B stores is stored, even when the sum is 0.0 or the term is 0 * a: alpha = 0 keeps
 *   A's pattern, and 0 * Inf is a NaN at its place.  A and B may have unsorted rows and repeated (row, col) pairs: each
 *   repeat is one more term, in stored order.  Rows of C ascend strictly and have no repeats, so hipSpILU0CSR, hipSpTRSVCSR
 *   and the serial-order SpMV selection accept C as it is.  The result is a function of the two handles' arrays, alpha and
 *   beta alone -- not of the run, the grid, the class a row fell into or the options.  Where a term is NaN, C has a NaN at
 *   that place; its payload is not pinned.  Every other value is pinned as bits: a -0.0 alone in its column gives +0.0
 *   (0.0 + -0.0), and a cancelling pair a stored +0.0.
 *   dC is like a product handle: u32 columns, 4-byte row pointers, its own unit detection, row blocks; every CSR entry
 *   point works on it; freed with hipFreeSpmat.  dA == dB is allowed.  Sources: spMatCpyCSR / spmvHipAdoptCSR (row
 *   pointers of 4 or 8 bytes) / transpose / permuted / product / sum handles, unit-value handles included.
 *   A row's class comes from t = its terms (entries of A's row + entries of B's row), from whether it is PLAIN (both stored
 *   rows ascend strictly) and from opts alone (NULL, or a field 0: the built-in default; a value above the built-in limit is
 *   clamped to it): plain and t <= laneMaxTerms (32, limit 64) one lane merges the two rows; plain and t <= waveMaxTerms
 *   (2 048, the limit) one wavefront places every entry by rank; everything else, and every row under allSorted, the
 *   sorted path of spmvHipSpGEMM (one stable radix sort per batch of rows whose terms fit sortBudgetBytes: 32 B per term,
 *   default 256 MiB, limit 4 GiB; a row above the budget is a batch of its own).
 *   Memory: C itself 12 B per entry + 4 B per row, its row blocks, and 4 B per row for the refresh (the rows by class).
 *   Temporaries, freed before the call returns: 20 B per row for the first pass and the lists (24 B with a row of more
 *   than 64 terms), then 12 B per row for the counts and their scan, 16 B per sorted row, and 32 B per term of the largest
 *   sorted batch + the sort's workspace.
 *   info: terms (entries of A + entries of B), nnzC, maxRowTerms, maxRowNnz, rowsLane / rowsWave / rowsSorted (they sum to
 *   the rows with a term), sortBatches, tempBytes (peak of the temporaries), symbolicMs / numericMs / ms (wall times).
 *   Synchronous on the library stream; allocates, so not capturable.  opts and info may be NULL.
 *   M = 0, N = 0, two empty sources and one empty source succeed with a valid C (NZ = 0 and SpMV +0.0 when both are empty).
 * spmvHipCsrAddRefresh recomputes C's values from the sources' CURRENT value arrays with the alpha and beta of THIS call
 *   (a shift sweep A - sigma I is one build and many refreshes), C's pattern and addresses kept: the numeric phase only, on
 *   the classes of the build, then what spmvHipValuesChanged(dC) does.  dC records both sources' ids in order (alpha goes
 *   with A) and refuses any other pair, and the same pair swapped.  The sources' patterns must be unchanged.
 * Refused with a message and EXIT_FAILURE, dC and info untouched: NULL dA, dB or dC; a handle that is not live; an ELL
 *   handle or a multigrid hierarchy; A.M != B.M or A.N != B.N; dC == dA or dC == dB; M or N >= 2^32 - 1; nnz(C) >=
 *   IRP32_LIMIT (2^32 - 65536; found after the symbolic phase, before C's column and value arrays exist); a column id >= N
 *   in a source (an adopted array; checked on the device in the first pass); a source with entries but no column or value
 *   array; a refresh of a handle that is not a sum, or from other sources. */
typedef struct {            /* 0 = the built-in default; a value above the built-in limit is clamped to it */
    ulong laneMaxTerms;     /* plain rows with at most this many terms: one lane each          */
    ulong waveMaxTerms;     /* ... at most this many: one wavefront each; above: the sorted path */
    ulong sortBudgetBytes;  /* temporaries of one batch of the sorted path                     */
    int   allSorted;        /* 1: every row on the sorted path (the general path, for checking) */
} spmvAddOpts;
typedef struct {
    ulong terms, nnzC, maxRowTerms, maxRowNnz;
    ulong rowsLane, rowsWave, rowsSorted, sortBatches;   /* the three sum to the rows with a term */
    ulong tempBytes;        /* peak of the build's temporaries */
    double symbolicMs, numericMs, ms;
} spmvAddInfo;
int spmvHipCsrAdd(double alpha, spmat* dA, double beta, spmat* dB, const spmvAddOpts* opts, spmat* dC, spmvAddInfo* info);
int spmvHipCsrAddRefresh(spmat* dC, double alpha, spmat* dA, double beta, spmat* dB, spmvAddInfo* info);
/* ------------------------------------------------------------- entry filter C = the kept entries of A */
/* spmvHipCsrFilter writes into dC a new, independent CSR handle that holds the entries of A a predicate keeps (tril / triu /
 * the diagonal for an L + D + U splitting, a drop tolerance, the strength-of-connection filter of smoothed aggregation).  The
 * contract is the bits of this serial loop on the handle's arrays (IRP, JA, AS as stored), DESIGN.md section 29:
 *       if STRENGTH or lump:  for i in 0 .. M-1:  d[i] = A.AS[p] of the ONE stored entry p of row i with A.JA[p] == i
 *       for i in 0 .. M-1:
 *           v = d[i]                                           (lump only)
 *           for p in A.IRP[i] .. A.IRP[i+1]-1:                 (A's stored order)
 *               j = A.JA[p];  a = A.AS[p]
 *               if keep(i, j, a):  append (j, a) to row i of C (a copied as bits), kept[next place of C] = p
 *               else if lump:      v = v + a                   (a plain add, in stored order)
 *           if lump:  the value of C's entry (i, i) = v        (its place does not move)
 *       keep(i, j, a), every product rounded, no FMA, a comparison with a NaN false:
 *           STRENGTH or lump, and j == i:  true                 (the diagonal entry is always kept)
 *           SPMV_FILTER_BAND:      opts->lo <= (int64_t)j - (int64_t)i && (int64_t)j - (int64_t)i <= opts->hi
 *           SPMV_FILTER_ABS:       fabs(a) > opts->theta
 *           SPMV_FILTER_STRENGTH:  a * a > (opts->theta * opts->theta) * fabs(d[i] * d[j])
 *   Order and values: row i of C is the kept entries of A's row i in A's stored order: unsorted rows stay unsorted, and each
 *   repeat of an (i, j) pair is judged on its own.  Values are copied as bits: -0.0 stays -0.0, a NaN keeps its payload; a
 *   NaN fails ABS and STRENGTH and is dropped (a NaN on the kept diagonal stays).  BAND is a function of the pattern alone:
 *   no value is read for the decision; lo > hi gives a valid empty C; INT64_MIN and INT64_MAX are the open ends, so
 *   tril is (INT64_MIN, 0), triu (0, INT64_MAX), the diagonal (0, 0).
 *   The diagonal d: STRENGTH, and lump in any mode, need a square A and the STORED rule of spmvHipAmgSetup: a row without
 *   exactly one stored entry (i, i) is refused, and the line names the first such row.
 *   lump = 1 (Vanek's filtered matrix; with ABS and STRENGTH): the loop above -- the sum v is the only arithmetic of the call.
 *   A dropped NaN or a dropped Inf lumps into its diagonal; where v is a NaN its payload is not pinned.  info.lumpedRows =
 *   the rows with at least one dropped entry.
 *   dC is like a sum handle: u32 columns, 4-byte row pointers, its own unit detection, row blocks; every CSR entry point
 *   works on it; freed with hipFreeSpmat.  Sources: spMatCpyCSR / spmvHipAdoptCSR (row pointers of 4 or 8 bytes) /
 *   transpose / permuted / product / sum / filtered handles, unit-value handles included.  The result is a function of A's
 *   arrays and opts alone -- not of the run or the grid.
 *   Memory: C itself 12 B per kept entry + 4 B per row, its row blocks, 4 B per kept entry for the refresh (kept[]), and
 *   with lump 1 bit per entry of A (the keep mask), 4 B per row (the diagonal's place in C) and 4 B per row of A above 64
 *   entries.  Temporaries, freed before the call returns: 1 bit per entry of A + 8 B per 1 024 entries, and 16 B per row
 *   where d is needed.  info: nnzA, nnzC, maxRowNnz (of C), lumpedRows, tempBytes (peak of the temporaries), ms (wall).
 *   Synchronous on the library stream; allocates, so not capturable.  info may be NULL.
 *   M = 0, N = 0, an empty A and a filter that keeps nothing succeed with a valid C (NZ = 0, SpMV +0.0).
 * spmvHipCsrFilterRefresh: the kept set is the BUILD's; nothing is judged again.  C.AS[q] = A.AS[kept[q]] from A's CURRENT
 *   values; with lump the diagonal is then the loop's v over A's current values at the build's dropped places.  C's pattern
 *   and device addresses stay; then what spmvHipValuesChanged(dC) does.  dC records A's id and refuses any other source.
 * Refused with a message and EXIT_FAILURE, dC and info untouched: NULL dA, opts or dC; a handle that is not live; an ELL
 *   handle or a multigrid hierarchy; dC == dA; an unknown mode; theta negative or not finite (in any mode); lump with
 *   BAND; STRENGTH or lump on a matrix that is not square, or that breaks the STORED rule; M or N >= 2^32 - 1; NZ >=
 *   IRP32_LIMIT (2^32 - 65536); a column id >= N in the source (an adopted array; checked on the device); a source with
 *   entries but no column or value array; a refresh of a handle that is not a filter, or from another source. */
#define SPMV_FILTER_BAND     0   /* keep (i, j) iff lo <= (int64)j - (int64)i <= hi                        */
#define SPMV_FILTER_ABS      1   /* keep iff fabs(a) > theta                                                */
#define SPMV_FILTER_STRENGTH 2   /* keep iff j == i, or a*a > (theta*theta) * fabs(d_i * d_j)               */
typedef struct {
    int     mode;           /* SPMV_FILTER_*                                                   */
    int64_t lo, hi;         /* BAND: the kept diagonals, INT64_MIN / INT64_MAX the open ends   */
    double  theta;          /* ABS, STRENGTH: the threshold                                    */
    int     lump;           /* 1: the dropped entries of a row are added to its diagonal entry */
} spmvFilterOpts;
typedef struct {
    ulong nnzA, nnzC, maxRowNnz, lumpedRows;
    ulong tempBytes;        /* peak of the build's temporaries */
    double ms;
} spmvFilterInfo;
int spmvHipCsrFilter(spmat* dA, const spmvFilterOpts* opts, spmat* dC, spmvFilterInfo* info);
int spmvHipCsrFilterRefresh(spmat* dC, spmat* dA, spmvFilterInfo* info);
/* ------------------------------------------------------------- assembly C = the sum of COO triplets */
/* spmvHipCooAssemble writes into dC a new, independent CSR handle assembled on the device from nEntries triplets
 * (dRow[e], dCol[e], dVal[e]) -- the element-matrix entries of a finite-element or finite-volume code: unsorted, a duplicate
 * per shared node, constrained rows and columns masked out with SPMV_COO_SKIP.  All three arrays are device memory.  The
 * contract is the bits of this serial loop, DESIGN.md section 36:
 *       kept = the entries e in 0 .. nEntries-1 with dRow[e] != SPMV_COO_SKIP and dCol[e] != SPMV_COO_SKIP   (ascending e)
 *       for i in 0 .. M-1:
 *           the distinct columns j of the kept entries with dRow[e] == i, ASCENDING  ->  row i of C
 *           for each such j, with e0 < e1 < ... < e_{r-1} the kept entries (i, j):
 *               SPMV_COO_SUM:   v = dVal[e0] (copied as bits);  for t in 1 .. r-1:  v = v + dVal[e_t]   (plain adds, no FMA)
 *               SPMV_COO_LAST:  v = dVal[e_{r-1}] (copied as bits)
 *               C.JA[q] = j, C.AS[q] = v
 *   Values: a sum of duplicates depends on its order in floating point, and "in input order" is the one order a caller can
 *   reproduce.  A single entry is copied as bits: -0.0 stays -0.0, a NaN keeps its payload; where a sum is a NaN its payload
 *   is not pinned.  Explicit zeros stay entries.  The pattern is a function of the indices alone: no value is read to decide
 *   it, and a value at a skipped place is never read at all.  C is a function of the arrays and opts alone -- not of the run
 *   or the grid.
 *   Cost: the duplicates of one (i, j) -- a run -- are added by ONE lane, because their order is the contract: a call costs
 *   at least its longest run, which info.maxRun reports.  There is no second, reordered path for long runs.
 *   dC is like a filtered handle: u32 columns, 4-byte row pointers, its own unit detection, row blocks; its rows ascend
 *   strictly, so ILU(0), the triangular schedules and the sum's merge path take them as they are; every CSR entry point works
 *   on it; freed with hipFreeSpmat.  The library keeps no pointer into dRow, dCol or dVal: the caller may free them when the
 *   call returns.  opts == NULL is {SPMV_COO_SUM, 1}.
 *   Memory: C itself 12 B per entry of C + 4 B per row and its row blocks; with keepMap = 1 the sorted order of the kept
 *   entries (4 B per kept entry) and the run starts (4 B per entry of C, + 4 B) for the refresh, nothing else; with keepMap
 *   = 0 nothing is kept.  Temporaries, freed before the call returns: 24 B per entry (two 64-bit keys and two entry indices
 *   for the sort's ping-pong) + the radix sort's workspace + 8 B per 1 024 kept entries, and without keepMap 4 B per entry of
 *   C.  info: nEntries, skipped, nnzC, duplicates (= nEntries - skipped - nnzC), maxRun (the most entries on one (i, j)),
 *   maxRowNnz (of C), tempBytes (peak of the temporaries), ms (wall).
 *   Synchronous on the library stream; allocates, so not capturable.  info may be NULL.
 *   M = 0, N = 0, nEntries = 0 and a list whose every entry is skipped succeed with a valid C (NZ = 0, SpMV +0.0); the
 *   arrays may be NULL when nEntries == 0.
 * spmvHipCooAssembleRefresh: new values for the SAME triplet list -- the same nEntries in the same order; the indices are
 *   not passed again.  C.AS[q] is the loop above over the build's runs, from the new dVal, in the build's mode; a value at a
 *   skipped place is never read.  C's pattern and device addresses stay; nothing is allocated for the assembly; then what
 *   spmvHipValuesChanged(dC) does (formats, unit detection, a pending ILU(0) dropped).  info: the build's counts, ms of this
 *   call, tempBytes 0.  spmvHipUpdateValues / spmvHipValuesChanged on an assembled handle behave as on a sum or a filtered one.
 * spmvHipCsrToCoo: dRow[p] = i, dCol[p] = JA[p], dVal[p] = AS[p] for the NZ entries p of any live CSR handle in stored order
 *   (row pointers of 4 or 8 bytes, unit-value handles included; dVal may be NULL: the pattern alone).  The arrays are the
 *   caller's device memory, NZ elements each; the library keeps no pointer to them.  Assembling its output reproduces a
 *   handle whose rows ascend strictly bit for bit.  Allocates nothing; synchronous on the library stream.
 * Refused with a "libspmvhip" line and EXIT_FAILURE, dC and info untouched, nothing held -- each of these before any launch
 *   or allocation: NULL dC; a NULL array with nEntries > 0; an unknown opts->duplicates; M or N >= 2^32 - 1; nEntries >=
 *   IRP32_LIMIT (2^32 - 65536).  A kept entry with dRow[e] >= M or dCol[e] >= N is found on the device, before C's column
 *   and value arrays exist: the line names the SMALLEST such e, its row and its column.  A refresh: a handle that was not made
 *   by spmvHipCooAssemble, or was built with keepMap = 0 (the line says so); another nEntries; a NULL dVal (with nEntries
 *   > 0).  spmvHipCsrToCoo: an ELL handle or a multigrid hierarchy; NULL dRow or dCol with NZ > 0; M >= 2^32 - 1.  No kernel
 *   is handed a pointer these checks have not passed. */
#define SPMV_COO_SKIP  0xFFFFFFFFu   /* an entry whose row OR column is this is left out */
#define SPMV_COO_SUM   0             /* duplicates of (i, j) are added in input order    */
#define SPMV_COO_LAST  1             /* the last duplicate in input order is the value   */
typedef struct {
    int duplicates;         /* SPMV_COO_SUM or SPMV_COO_LAST                                   */
    int keepMap;            /* 1: keep the sorted order and the run starts for a refresh       */
} spmvCooOpts;
typedef struct {
    ulong nEntries, skipped, nnzC, duplicates, maxRun, maxRowNnz;   /* duplicates = nEntries - skipped - nnzC */
    ulong tempBytes;        /* peak of the build's temporaries */
    double ms;
} spmvCooInfo;
int spmvHipCooAssemble(ulong M, ulong N, ulong nEntries, const uint32_t* dRow, const uint32_t* dCol, const double* dVal,
                       const spmvCooOpts* opts, spmat* dC, spmvCooInfo* info);
int spmvHipCooAssembleRefresh(spmat* dC, ulong nEntries, const double* dVal, spmvCooInfo* info);
int spmvHipCsrToCoo(spmat* dA, uint32_t* dRow, uint32_t* dCol, double* dVal);
/* ------------------------------------------------------------- aggregation multigrid preconditioner */
/* Plain (unsmoothed) aggregation AMG built from the pieces above: an aggregation of the pattern, the Galerkin products by
 * spmvHipCsrTranspose / spmvHipSpGEMM, a damped-Jacobi V-cycle on serial-order SpMVs.  DESIGN.md section 24.  As everywhere
 * in this header the result is a function of the handle's arrays and the options alone, and every number is the bits of a
 * loop written here.
 *
 * spmvHipAggregateCSR: dAgg[i] (M words) = the aggregate of vertex i of a square CSR handle.  A function of the PATTERN and
 *   the seed alone.  adj(i) is the one of spmvHipColourCSR (the pattern of A + A^T, the diagonal ignored, repeats counted
 *   once, unsorted rows allowed, column ids >= M skipped); key(i) = fmix32(i ^ seed); j beats i iff (key(j), j) > (key(i), i)
 *   (the HASH order of spmvHipColourCSR).  dist(i, j) is the path length in adj.
 *       roots:     for i in descending (key, id):  i is a root iff no root chosen so far has dist(i, root) <= 2
 *                  (the lexicographically first distance-2 maximal independent set; a vertex with empty adj is a root)
 *       numbering: id(root r) = the number of roots with a smaller row id
 *       ring 1:    a non-root i with a root r in adj(i):  agg[i] = id(r)            (there is at most one such root)
 *       ring 2:    every other i:  agg[i] = agg[k], k the ring-1 vertex of adj(i) that beats all other ring-1 vertices of
 *                  adj(i)                                                            (one exists: the set is maximal)
 *   The device runs rounds: every undecided vertex that beats all undecided vertices within distance 2 becomes a root, then
 *   everything within distance 2 of a new root retires; a distance-2 path counts whatever its middle vertex is (undecided,
 *   retired).  Only info.rounds may differ between runs.  Rows with more than 64 adjacency entries take a wavefront each,
 *   the others a lane.  info: aggregates, rounds, hostChecks (one read-back per K rounds, K = 16 unless
 *   spmvHipSetVariant("spmvHipAggregateCSR", K), 1 <= K <= 4096), longRows, symmetric (as spmvColourInfo), maxAggRows /
 *   minAggRows (the largest and smallest aggregate; 0 when M = 0), ms.  opts == NULL: seed 0.  Synchronous on the library
 *   stream; allocates, so not capturable; temporaries freed before it returns.  M = 0 succeeds, nothing written.
 *   Refusals: those of spmvHipColourCSR (a handle that is not live, ELL, M != N, M >= 2^31 or NZ >= IRP32_LIMIT), and a NULL
 *   dAgg when M > 0.  After a failed device allocation ("refused allocations" above) info is unwritten, but dAgg may have
 *   been written in part and holds nothing to rely on.
 *
 * spmvHipAmgSetup writes into dM a handle of its own kind: a hierarchy.  It is no matrix -- every SpMV, format, build and
 *   solve entry point refuses it with a message -- and is freed by hipFreeSpmat.  It records dA's id and keeps no pointer to
 *   it.  With A_0 = A, for l = 0, 1, ...:
 *       dinv_l[i] = 1.0 / (the one stored entry (i, i) of A_l)       (a row without exactly one: refused, the STORED rule)
 *       stop (l is the last level) when M_l <= coarseRows, or l + 1 == maxLevels
 *       agg_l = spmvHipAggregateCSR(A_l, seed);  stop when nAgg_l == M_l
 *       P_l = the M_l x nAgg_l CSR handle with the one entry (i, agg_l[i]) = 1.0 per row        (a unit-value handle)
 *       R_l = spmvHipCsrTranspose(P_l);  A_{l+1} = spmvHipSpGEMM(R_l, spmvHipSpGEMM(A_l, P_l))
 *   so A_{l+1}'s arrays are what those calls give (rows ascend strictly).  A_l P_l is kept: the refresh of A_{l+1} reads it.
 *   P_l and R_l keep their value arrays of 1.0 (8 B per row of A_l each, counted in info.bytes): their SpMVs stream no
 *   values, but the products and their refreshes read the value arrays of their operands.
 *   opts (NULL, or a field 0: the built-in default): seed; coarseRows 512; maxLevels 16 (at most SPMV_AMG_MAX_LEVELS);
 *   omega 2/3; nu1 1, nu2 1, nuCoarse 8 sweeps -- SPMV_AMG_NO_SWEEPS asks for none, 0 being the default.  The defaults are
 *   conventions.  The workspace of the cycle (t, d per level, r, z below level 0) is allocated here, and every level's
 *   serial-order SpMV selection is made here, dA's included.  info (also spmvHipAmgInfo): levels, rows / nnz / aggregates per
 *   level (aggregates 0 on the last), opComplexity = sum nnz_l / nnz_0, bytes kept, tempBytes (the largest of the products'
 *   temporaries), ms.  Synchronous; allocates.
 * spmvHipAmgLevel: a view of level l for inspection: *dAl = a copy of A_l's spmat with dev = NULL (its arrays stay dM's;
 *   level 0: only M, N, NZ are set), *dAgg = agg_l (NULL on the last level), *dDinv = dinv_l.  Any of the three may be NULL.
 * spmvHipAmgRefresh: dA has new values on the same pattern: spmvHipSpGEMMRefresh down the chain and every dinv again;
 *   aggregates, P and R stay.  Bit-identical to a fresh setup.
 * spmvHipAmgApply: dZ = V(0, dR), in IEEE double, no FMA, every operation rounded in the order written; A v is level l's
 *   serial-order SpMV (spmvHipEnqueueAutoRows), L the number of levels:
 *       V(l, r) -> z:
 *         sweeps = (l == L-1) ? nuCoarse : nu1
 *         if sweeps == 0: z_i = +0.0
 *         else first sweep (no SpMV):  z_i = omega * (dinv_i * r_i)
 *              each further sweep:     t = A_l z;  z_i = z_i + omega * (dinv_i * (r_i - t_i))        (Jacobi: t from the old z)
 *         if l == L-1: return z
 *         t = A_l z;  d_i = r_i - t_i;  rc = R_l d (serial-order SpMV on the transpose handle);  e = V(l+1, rc)
 *         z_i = z_i + e[agg_l[i]]                              (a gather, NOT an SpMV with P_l: the two differ at -0.0)
 *         nu2 times:  t = A_l z;  z_i = z_i + omega * (dinv_i * (r_i - t_i))
 *   Kernels only, on the library stream, no allocation: capturable; honours spmvHipSetSync.  dR and dZ need 8-byte
 *   alignment only.  dA must be the handle of the setup, with the values of the setup or of the last refresh.
 *   One cycle enqueues, with s(n) = 1 + 2 * (max(n, 1) - 1) kernels for n sweeps from nothing (an SpMV counted as one),
 *       (L - 1) * (s(nu1) + 3 + 1 + 2 * nu2) + s(nuCoarse)
 *   kernels: the residual's SpMV and pass and the restriction, the gather, two per further sweep.
 *   A hierarchy has ONE workspace: every Apply and every solve with it as dM uses the same vectors.  Two of them running at
 *   once -- on two streams, or a replayed capture beside a call -- race; keep them in stream order or synchronised.
 * As dM of hipSpCGCSR / hipSpBiCGStabCSR / hipSpGMRESCSR: see there.
 * Refused with a message and EXIT_FAILURE, outputs untouched: NULL dA, dM, dR or dZ; handles that are not live; for the
 *   setup the refusals of spmvHipAggregateCSR, dM == dA, a source without column or value array, a row without exactly one
 *   stored diagonal entry, omega negative or not finite, maxLevels > SPMV_AMG_MAX_LEVELS; a dM that is not a hierarchy; a
 *   dA that is not the source; dR and dZ overlapping; a level beyond the last.
 *
 * Smoothed aggregation.  spmvHipAmgSetupSmoothed writes a hierarchy of the same kind -- freed by
 *   hipFreeSpmat, refused by every matrix entry point, taken by spmvHipAmgApply / Refresh / Info / Level and as dM of
 *   hipSpCGCSR / hipSpBiCGStabCSR / hipSpGMRESCSR; the block solvers refuse it like any hierarchy -- whose prolongator is
 *   damped-Jacobi smoothed.  opts, dinv_l, the stop rules and agg_l are those of spmvHipAmgSetup; per level that is not the last:
 *       T_l  = the unit-value M_l x nAgg_l handle with the one entry (i, agg_l[i]) = 1.0 per row   (spmvHipAmgSetup's P_l)
 *       s_i  = +0.0; for p in A_l.IRP[i] .. A_l.IRP[i+1]-1 (stored order): s_i = s_i + fabs(A_l.AS[p])
 *       g_i  = fabs(dinv_l[i]) * s_i;   rho_l = max_i g_i
 *       w_l  = smooth->omegaP != 0 ? smooth->omegaP : (4.0 / 3.0) / rho_l             (two rounded divisions, as written)
 *       D_l  = the M_l x M_l CSR handle with the one entry (i, i) = dinv_l[i] per row
 *       P_l  = spmvHipCsrAdd(1.0, T_l, -w_l, spmvHipSpGEMM(D_l, spmvHipSpGEMM(A_l, T_l)))
 *       R_l  = spmvHipCsrTranspose(P_l);   A_{l+1} = spmvHipSpGEMM(R_l, spmvHipSpGEMM(A_l, P_l))
 *   Every array of P_l, R_l and A_{l+1} is what those calls give; only s_i, g_i and w_l are arithmetic of this entry point
 *   (the max of non-negative doubles does not depend on its order).  smooth == NULL: omegaP = 0.  On the 7-point Laplacian
 *   the default gives w_0 = 2/3 exactly.  T_l, D_l, A_l T_l, D_l (A_l T_l) and A_l P_l are kept (the refresh reads them) and
 *   counted in info.bytes; info.tempBytes also covers the sums' temporaries; the other fields mean what they mean above.
 *   Refused besides what spmvHipAmgSetup refuses, outputs untouched: an omegaP that is negative or not finite; a level with
 *   a g_i that is not finite, or with rho_l = 0 (the line names the first such row and its level).
 *   The cycle is V(l, r) above with its correction line replaced by
 *       for each i:  s = +0.0;  for p in P_l.IRP[i] .. P_l.IRP[i+1]-1 (stored order):  s = s + P_l.AS[p] * e[P_l.JA[p]]
 *                    z_i = z_i + s
 *   the serial-order SpMV with P_l followed by an add, no FMA.  A level whose P_l has no row longer than n entries does it in
 *   ONE kernel (a lane walks two rows of P_l); a level with a longer row in two, spmvHipEnqueueAutoRows(P_l, e, d) and
 *   z = z + d (the same bits).  n = 0 (never fused: the two-kernel form measured faster) unless
 *   spmvHipSetVariant("spmvHipAmgApply", n), 0 <= n <= 4096 (64 is the long-row convention of the other kernels), read at the
 *   SETUP, so Apply still only enqueues: kernels only, capturable, no allocation.  One cycle enqueues
 *       (L - 1) * (s(nu1) + 3 + 1 + 2 * nu2) + s(nuCoarse) + (the levels whose correction is not fused)
 *   kernels.  A hierarchy of spmvHipAmgSetup keeps its gather, its bits and its count.
 *   spmvHipAmgRefresh on a smoothed hierarchy: per level dinv_l, rho_l and w_l, D_l's values, then the refreshes of
 *   A_l T_l, D_l (A_l T_l), P_l (spmvHipCsrAddRefresh with the new w_l), R_l, A_l P_l and A_{l+1}; aggregates and every
 *   pattern stay (all patterns are structural), device addresses are kept.  Bit-identical to a fresh setup.
 * spmvHipAmgProlongator: a view like spmvHipAmgLevel's of a level that is not the last: *dPl, *dRl = copies of P_l's and
 *   R_l's spmat with dev = NULL (the arrays stay dM's), *omegaP = w_l.  Any of the three may be NULL.  On a hierarchy of
 *   spmvHipAmgSetup: the unit P_l, its R_l and 0.0.  Refused: a dM that is not a hierarchy, the last level and beyond.
 *
 * Strength-filtered smoothed aggregation.  spmvHipAmgSetupStrength writes a smoothed hierarchy -- every
 *   sentence above about spmvHipAmgSetupSmoothed's handle, cycle, launch counts and views holds -- that aggregates on, and
 *   smooths its prolongator with, the strength-filtered matrix, so that on an anisotropic operator the aggregates follow the
 *   strong direction.  opts and smooth are those of spmvHipAmgSetupSmoothed.  strength (NULL, or a field 0: the default):
 *   theta 0.08, thetaScale 0.5; theta_0 = theta, theta_{l+1} = theta_l * thetaScale (one rounded product per level: a fixed
 *   theta stalls on the coarse levels, whose entries are more alike).  Per level that is not the last:
 *       F_l   = spmvHipCsrFilter(A_l, {SPMV_FILTER_STRENGTH, theta = theta_l, lump = 1})
 *       agg_l = spmvHipAggregateCSR(F_l, seed);   stop when nAgg_l == M_l          (F_l is then dropped)
 *       dF_l[i] = 1.0 / (the stored entry (i, i) of F_l);   s_i, g_i, rho_l, w_l as above, from F_l's rows and dF_l
 *       D_l   = the M_l x M_l CSR handle with the one entry (i, i) = dF_l[i] per row
 *       P_l   = spmvHipCsrAdd(1.0, T_l, -w_l, spmvHipSpGEMM(D_l, spmvHipSpGEMM(F_l, T_l)))
 *       R_l   = spmvHipCsrTranspose(P_l);   A_{l+1} = spmvHipSpGEMM(R_l, spmvHipSpGEMM(A_l, P_l))     (Galerkin on the FULL A_l)
 *   dinv_l, and with it the Jacobi sweeps of the cycle, stay those of A_l.  F_l and dF_l are kept and counted in info.bytes.
 *   theta = 1e-200 (theta * theta is 0.0) keeps every nonzero entry: on a matrix without a stored zero the arrays are
 *   spmvHipAmgSetupSmoothed's.
 *   spmvHipAmgRefresh on such a hierarchy runs spmvHipCsrFilterRefresh(F_l, A_l) first, then dF_l and the smoothed chain
 *   above with F_l in A_l's place.  The kept sets and the aggregates are the BUILD's: the refreshed hierarchy equals a fresh
 *   setup bit for bit WHEN A FRESH SETUP WOULD KEEP THE SAME ENTRIES (all values scaled by a power of two, say); otherwise it
 *   is the hierarchy of the build's pattern with the new values -- a valid preconditioner, not the fresh one.
 *   Refused besides what spmvHipAmgSetupSmoothed refuses, outputs untouched: theta or thetaScale negative or not finite;
 *   thetaScale > 1.
 * spmvHipAmgStrength: a view like spmvHipAmgProlongator's of a level that is not the last: *dFl = a copy of F_l's spmat with
 *   dev = NULL (the arrays stay dM's), *theta = theta_l.  Either may be NULL.  Refused: a dM that is not a hierarchy of
 *   spmvHipAmgSetupStrength, the last level and beyond.
 *
 * Chebyshev smoother of the cycle.  spmvHipAmgSetSmoother(dM, dA, opts) chooses what a hierarchy of
 *   any of the three setups smooths with, and how often: it changes what spmvHipAmgApply, and every Krylov loop that takes
 *   the hierarchy as dM, enqueues FROM THEN ON -- a cycle captured earlier must be captured again.  Synchronous on the library
 *   stream; it allocates the coefficient tables (and nothing else), so it is not capturable.  opts (NULL, or a field 0: the
 *   built-in default): kind JACOBI; nu1, nu2, nuCoarse 0: the hierarchy's current counts, SPMV_AMG_NO_SWEEPS: none, at most
 *   SPMV_AMG_MAX_DEGREE otherwise; eigRatio 10 (a convention); lambdaScale 1.0.  The counts apply to both kinds: with kind
 *   JACOBI the call changes the sweeps of a Jacobi hierarchy without a new setup, and the cycle is V(l, r) above, its bits and
 *   its kernel count, for those counts.  A hierarchy on which the call was never made is untouched in every respect.
 *   With kind CHEBYSHEV, per level l (the last included; on a strength hierarchy from A_l, NOT F_l: the sweeps are A_l's):
 *       rho_l = max_i fabs(dinv_l[i]) * s_i, s_i the sum of fabs(A_l.AS[p]) over row i in stored order from +0.0  (as above)
 *       lmax = lambdaScale * rho_l;   lmin = lmax / eigRatio
 *       theta = (lmax + lmin) / 2.0;  delta = (lmax - lmin) / 2.0;  sigma = theta / delta
 *       s_0 = 1.0 / sigma;            a_0 = 0.0;   b_0 = 1.0 / theta
 *       k >= 1:  s_k = 1.0 / (2.0 * sigma - s_{k-1});   a_k = s_k * s_{k-1};   b_k = (2.0 * s_k) / delta
 *   for k < max(nu1, nu2), on the last level k < nuCoarse -- computed on the host in IEEE double, every operation rounded in
 *   the order written (2.0 * sigma - s is a product, then a difference); a numpy float64 transcription gives the same bits.
 *   rho_l = ||D^-1 A||_inf bounds lambda_max(D^-1 A) for any matrix and does not depend on a summation order.  The pairs
 *   (a_k, b_k) of a level live in device memory and the kernels read them there (one uniform 16-byte load), so a captured
 *   cycle replayed after spmvHipAmgRefresh uses the new coefficients.  A level without rows has rho_l = 0 and zeros.
 *   The smoother, d the level's d_l (free at both places; no new vector), no FMA:
 *       Cheb(l, r, z, q, fromNothing):
 *         k = 0, fromNothing:  d_i = b_0 * (dinv_i * r_i);                          z_i = d_i          (no SpMV)
 *         k = 0, otherwise:    t = A_l z;  d_i = b_0 * (dinv_i * (r_i - t_i));      z_i = z_i + d_i
 *         k = 1 .. q-1:        t = A_l z;  d_i = a_k * d_i + b_k * (dinv_i * (r_i - t_i));   z_i = z_i + d_i
 *   and the cycle is V(l, r) above with its pre-smoothing lines replaced by Cheb(l, r, z, sweeps, true) (z_i = +0.0 when
 *   sweeps == 0) and its nu2 lines by Cheb(l, r, z, nu2, false): the recurrence RESTARTS at k = 0 there.  The residual, the
 *   restriction and the correction (gather, P e in both forms, the fuse threshold) are unchanged, and so is the kernel count:
 *   a Chebyshev step is one SpMV and one pass, like a sweep.
 *   spmvHipAmgRefresh on a Chebyshev hierarchy recomputes, after dinv_l, rho_l and the table of every level and writes the
 *   table to the same device address: bit-identical to a fresh setup followed by the same spmvHipAmgSetSmoother.  A rho_l
 *   that is 0 or not finite refuses the refresh with the line below; a later refresh with good values recovers.
 *   spmvAmgInfo.bytes counts the tables (16 B per pair).
 *   Refused with a message and EXIT_FAILURE, the hierarchy, its smoother and its tables exactly as they were: NULL dM or dA;
 *   handles that are not live; a dM that is not a hierarchy; a dA that is not the source; an unknown kind; an eigRatio that is
 *   not finite or is <= 1 (0 excepted: the default); a lambdaScale that is negative or not finite; a count above
 *   SPMV_AMG_MAX_DEGREE other than SPMV_AMG_NO_SWEEPS; with CHEBYSHEV a level whose rho_l is 0 or not finite (the line names
 *   the level and the first such row).
 * spmvHipAmgSmoother: a view of level l: kind, the counts in force (0: none), rho_l, lambdaMax, lambdaMin, nCoef and dCoef =
 *   the device address of the nCoef pairs (a_0, b_0, a_1, b_1, ...; NULL when nCoef = 0).  On a hierarchy never given a
 *   smoother, or given JACOBI: kind JACOBI, the counts, zeros and NULL.  Refused, info untouched: a dM that is not a
 *   hierarchy, a level beyond the last, a NULL info.
 *
 * Multicolour Gauss-Seidel smoother of the cycle.  spmvHipAmgSetGaussSeidel(dM, dA, opts) makes a
 *   hierarchy of any of the three setups smooth with Gauss-Seidel sweeps ordered by a colouring, FROM THEN ON, as
 *   spmvHipAmgSetSmoother does for its two kinds (a cycle captured earlier must be captured again; synchronous on the
 *   library stream; it allocates the colour lists and nothing else, so it is not capturable).  It is an entry point of its
 *   own: spmvHipAmgSetSmoother keeps refusing kind 2.  opts (NULL, or a field 0: the built-in default): order NATURAL, seed,
 *   omega 1.0, oneWay 0 (symmetric), levels 0 (all), nu1 / nu2 / nuCoarse as in spmvAmgSmootherOpts.  The defaults are
 *   conventions.  Per Gauss-Seidel level l, l < levels (on a strength hierarchy from A_l, NOT F_l: the sweeps are A_l's):
 *       colour_l, perm_l = what spmvHipColourCSR(A_l, {order, seed}) gives;   C_l = its colour count
 *       dColourPtr = the C_l + 1 offsets of the colour classes in perm_l     (class c is perm_l[dColourPtr[c] .. dColourPtr[c+1]-1])
 *   Rows of one colour store no column of that colour but their own diagonal (a colouring of A + A^T), so the rows of a colour
 *   may run in any order and on any lane.  The smoother, no FMA, every operation rounded in the order written:
 *       GS(l, r, z, q, fromNothing, backward_k):
 *         if fromNothing:  z_i = +0.0 for every i
 *         for k = 0 .. q-1:
 *           for c = 0 .. C_l-1  (backward_k: C_l-1 .. 0):
 *             for every row i of colour c:
 *               t = +0.0;  for p in A_l.IRP[i] .. A_l.IRP[i+1]-1 (stored order):  t = t + A_l.AS[p] * z[A_l.JA[p]]
 *               z_i = z_i + omega * (dinv_i * (r_i - t))
 *   the Jacobi sweep's line with the serial-order row sum taken from the CURRENT z, one colour at a time.  The cycle is V(l, r)
 *   above with, on a Gauss-Seidel level, the pre-smoothing lines replaced by GS(l, r, z, sweeps, true, forward) (sweeps == 0
 *   still gives z = +0.0) and the nu2 lines by GS(l, r, z, nu2, false, oneWay ? forward : backward); on the last level sweep k
 *   runs forward when oneWay or k is even, backward otherwise.  The residual, the restriction, the correction (gather, fused
 *   or two-kernel P e) and the stop pointer are unchanged.  Levels l >= levels run the Jacobi lines of V with the hierarchy's
 *   omega, bit for bit.  With oneWay = 0 and nu1 = nu2 the cycle is a symmetric operator for a symmetric A (what CG needs).
 *   Kernels.  A sweep of a level is one launch per colour, whatever the row lengths.  A row takes g lanes, which form g
 *   products at a time from consecutive entries while the additions stay in stored order (the bits fix the order of the
 *   additions, not the lane that performs them): g = the largest power of two from 4 to 64 that the level's mean row fills
 *   (1 on a level whose mean is at most 2), unless spmvHipSetVariant("spmvHipAmgGaussSeidel", g), g = 1, 4, 8, 16, 32 or 64
 *   (0: by the mean again), read at the SET call; with g = 1 a row of at most 64 stored entries takes a lane and a longer
 *   one a wavefront (the convention of the colouring and the aggregation).  The same bits for every g.  A SMALL
 *   level, 0 < M_l <= n, runs a whole sweep -- all colours in order, a workgroup barrier between them -- in ONE launch of one
 *   workgroup: the same bits.  n = 1024 (a convention) unless spmvHipSetVariant("spmvHipAmgSetGaussSeidel", n), 0 <= n <=
 *   65536, 0: never; read at the SET call, so Apply still only enqueues: kernels only, capturable, no allocation.  With
 *   K_l = 1 for a small level, C_l otherwise, 0 when M_l = 0, the Gauss-Seidel levels of one cycle enqueue
 *       sum over l < L-1 of (1 + nu1 * K_l + 3 + 1 [+ 1 when the correction is not fused] + nu2 * K_l)  +  1 + nuCoarse * K_{L-1}
 *   kernels (the zero pass, the sweeps, the residual's SpMV and pass and the restriction, the correction); a Jacobi level
 *   keeps its term of the formulas above.  Ordering comes from kernel boundaries and that barrier alone.
 *   Kept per Gauss-Seidel level and counted in spmvAmgInfo.bytes: perm_l (4 B per row) and dColourPtr (4 (C_l + 1) B); no new
 *   vector.  spmvHipAmgRefresh recomputes nothing for this smoother beyond dinv_l -- the colours are the pattern's -- and
 *   keeps the addresses: a refreshed hierarchy is bit-identical to a fresh setup followed by the same call, and a captured
 *   cycle replayed after a refresh is valid.
 *   Switching: spmvHipAmgSetSmoother(JACOBI | CHEBYSHEV) on a Gauss-Seidel hierarchy drops the colour lists (the bytes of a
 *   hierarchy that never had them); spmvHipAmgSetGaussSeidel on a Chebyshev hierarchy drops the tables, on a Gauss-Seidel
 *   hierarchy the old lists.  Everything new is made before anything old is dropped.  spmvHipAmgSmoother on a Gauss-Seidel
 *   hierarchy reports kind SPMV_AMG_SMOOTHER_GAUSS_SEIDEL, the counts, zeros and NULL.
 *   Refused with a message and EXIT_FAILURE, the hierarchy, its smoother and its views exactly as they were: NULL dM or dA;
 *   handles that are not live; a dM that is not a hierarchy; a dA that is not the source; an unknown order; an omega that is
 *   not finite or is < 0 (0: the default); a count above SPMV_AMG_MAX_DEGREE other than SPMV_AMG_NO_SWEEPS.
 * spmvHipAmgGaussSeidel: a view of level l: active (1 on a Gauss-Seidel level), colours = C_l, maxColourRows, longRows (the
 *   rows of A_l above 64 stored entries), small (1: the one-workgroup sweep), omega, order, seed, oneWay, dPerm and dColourPtr
 *   (device addresses, the hierarchy's).  On a Jacobi level of a Gauss-Seidel hierarchy, and on a hierarchy that smooths
 *   otherwise: zeros and NULL.  Refused, info untouched: a dM that is not a hierarchy, a level beyond the last, a NULL info.
 *
 * The cycle for a block of vectors.  Opt-in per hierarchy: a block cycle needs a workspace of its
 *   own, because Apply must not allocate, and a hierarchy that was never given one is refused by the block entry points
 *   as before.
 * spmvHipAmgSetBlockWidth(dM, dA, width) gives a hierarchy of any of the three setups the workspace of a block cycle for up
 *   to `width` columns: per level t_l and d_l, below level 0 also r_l and z_l, each an M_l x kp row-major block, kp = width
 *   rounded up to even, 16-byte aligned: 8 kp (2 M_0 + 4 (M_1 + ... + M_{L-1})) bytes in all.
 *   width = 0 drops it: the hierarchy is then, in every respect and in spmvAmgInfo.bytes, one that never had it.  A second
 *   call replaces the width; everything new is made before anything old is dropped.  Synchronous on the library stream; it
 *   allocates, so it is not capturable.  The workspace holds no values: spmvHipAmgRefresh, spmvHipAmgSetSmoother and
 *   spmvHipAmgSetGaussSeidel keep it and its addresses.  spmvAmgInfo.bytes counts it; spmvHipAmgBlock reports the width
 *   and its bytes alone (zeros on a hierarchy without; refused, info untouched: a dM that is not a hierarchy, a NULL info).
 *   The single-vector workspace, spmvHipAmgApply and the single solves are untouched: same bits, same launch counts.  The
 *   block workspace is ONE, like the single one: two block cycles at once race; keep them in stream order.
 *   Refused with a message and EXIT_FAILURE, the hierarchy exactly as it was: a NULL or not-live handle; a dM that is not a
 *   hierarchy; a dA that is not the source; a size M_0 * kp * 8 that overflows, or an allocation that fails.
 * spmvHipAmgApplyBlock: Z(:, c) = V(0, R(:, c)) for c = 0 .. k-1.  R and Z are M x k on the device, each with its own
 *   layout and leading dimension by the rules of hipSpMMRowsCSR / hipSpTRSMCSR; only 8-byte alignment is needed.
 *   Bits: every column of Z is bit for bit spmvHipAmgApply(dM, dA, R(:, c)) -- the loops V and Cheb and the P e correction
 *   above -- for Jacobi and Chebyshev hierarchies of all three setups, whatever k, the layouts, the leading dimensions and
 *   the alignment are.  Columns are independent: a NaN, an Inf or a -0.0 in one never reaches another.  Elements outside
 *   the M x k block of Z are never written; R is only read.
 *   Execution: the loop of the single cycle with every A_l z, R_l d and P_l e one hipSpMMRowsCSR pass on the level's handle
 *   (a pass over more than 16 columns is several launches counted as one) and every fused vector pass one block launch
 *   covering all columns (a workgroup per 4096 rows and 16-column panel).  The plain correction is the gather
 *   Z(i, c) = Z(i, c) + E(agg_l[i], c), not a product with P_l (the two differ at -0.0, as in the single cycle); a smoothed
 *   or strength hierarchy always corrects in two kernels, the product with P_l into d_l and Z = Z + d_l: the fuse threshold
 *   of spmvHipSetVariant("spmvHipAmgApply", n) does not apply to the block cycle.  Chebyshev reads the same per-level table
 *   in device memory: a captured block cycle replayed after a refresh uses the new coefficients.  With s(q) = 2 q - 1 for
 *   q >= 1 and s(0) = 1, one block cycle enqueues
 *       (L - 1) * (s(nu1) + 3 + 1 + 2 * nu2) + s(nuCoarse) + (L - 1 on a smoothed or strength hierarchy)
 *   launches whatever k is: the formula above with no level fused.  Kernels only, on the library stream, no allocation:
 *   capturable; it honours spmvHipSetSync.  k = 1 takes the same path (no shortcut to the single cycle).  M = 0 succeeds
 *   with no kernel.  The padding column of the workspace (k odd) carries unspecified values; it is never stored into a
 *   caller's block and never influences a real column.
 *   Refused with a message and EXIT_FAILURE, Z untouched: NULL pointers; handles that are not live; a dM that is not a
 *   hierarchy; a dA that is not the source; k = 0; an unknown layout; a leading dimension too small for its layout; any
 *   overlap of the address spans of R and Z (the checks of hipSpTRSMCSR; there is no in-place form); a hierarchy without a
 *   block workspace or with width < k (the line contains "multigrid hierarchy", names spmvHipAmgSetBlockWidth and gives
 *   the width and k); a hierarchy with a Gauss-Seidel level (the line contains "multigrid hierarchy" and "Gauss-Seidel":
 *   the block form of the colour sweeps does not exist; the width is kept, and after spmvHipAmgSetSmoother(JACOBI |
 *   CHEBYSHEV) the block cycle works again). */
#define SPMV_AMG_SMOOTHER_JACOBI     0
#define SPMV_AMG_SMOOTHER_CHEBYSHEV  1
#define SPMV_AMG_SMOOTHER_GAUSS_SEIDEL 2      /* reported by the views; set only by spmvHipAmgSetGaussSeidel */
#define SPMV_AMG_MAX_DEGREE          64
#define SPMV_AMG_MAX_LEVELS 16
#define SPMV_AMG_NO_SWEEPS  0xFFFFFFFFu
typedef struct {
    uint32_t seed;          /* of the keys                                                   */
} spmvAggOpts;
typedef struct {
    ulong  aggregates;
    ulong  rounds;          /* rounds until every vertex was a root or retired               */
    ulong  hostChecks;      /* read-backs of the device state                                */
    ulong  longRows;        /* rows handled by a wavefront each                              */
    int    symmetric;       /* 1: stored pattern symmetric, transposed pattern not built     */
    ulong  maxAggRows;
    ulong  minAggRows;
    double ms;
} spmvAggInfo;
typedef struct {            /* 0 = the built-in default */
    uint32_t seed;
    ulong    coarseRows;    /* a level with at most this many rows is the last (512)         */
    unsigned maxLevels;     /* levels at most (16)                                           */
    double   omega;         /* Jacobi damping (2/3)                                          */
    unsigned nu1;           /* sweeps before the coarse correction (1)                       */
    unsigned nu2;           /* ... after it (1)                                              */
    unsigned nuCoarse;      /* sweeps on the last level (8); SPMV_AMG_NO_SWEEPS: none        */
} spmvAmgOpts;
typedef struct {
    unsigned levels;
    ulong  rows[SPMV_AMG_MAX_LEVELS];
    ulong  nnz[SPMV_AMG_MAX_LEVELS];
    ulong  aggregates[SPMV_AMG_MAX_LEVELS];
    double opComplexity;    /* sum of nnz over the levels / nnz of level 0                   */
    ulong  bytes;           /* device memory the hierarchy keeps                             */
    ulong  tempBytes;       /* the largest temporaries of one product of the build           */
    double ms;
} spmvAmgInfo;
int spmvHipAggregateCSR(spmat* dA, const spmvAggOpts* opts, uint32_t* dAgg, spmvAggInfo* info);
int spmvHipAmgSetup(spmat* dA, const spmvAmgOpts* opts, spmat* dM, spmvAmgInfo* info);
int spmvHipAmgRefresh(spmat* dM, spmat* dA);
int spmvHipAmgApply(spmat* dM, spmat* dA, const double* dR, double* dZ);
int spmvHipAmgInfo(spmat* dM, spmvAmgInfo* info);
int spmvHipAmgLevel(spmat* dM, unsigned level, spmat* dAl, const uint32_t** dAgg, const double** dDinv);
typedef struct {            /* 0 = the built-in default */
    double omegaP;          /* prolongator damping; 0: per level (4/3) / rho_l; else used on every level */
} spmvAmgSmoothOpts;
int spmvHipAmgSetupSmoothed(spmat* dA, const spmvAmgOpts* opts, const spmvAmgSmoothOpts* smooth, spmat* dM, spmvAmgInfo* info);
int spmvHipAmgProlongator(spmat* dM, unsigned level, spmat* dPl, spmat* dRl, double* omegaP);
typedef struct {            /* 0 = the built-in default */
    double theta;           /* the strength threshold of level 0 (0.08)                      */
    double thetaScale;      /* theta_{l+1} = theta_l * thetaScale (0.5); at most 1           */
} spmvAmgStrengthOpts;
int spmvHipAmgSetupStrength(spmat* dA, const spmvAmgOpts* opts, const spmvAmgSmoothOpts* smooth,
                            const spmvAmgStrengthOpts* strength, spmat* dM, spmvAmgInfo* info);
int spmvHipAmgStrength(spmat* dM, unsigned level, spmat* dFl, double* theta);
typedef struct {            /* 0 = the built-in default */
    int      kind;          /* SPMV_AMG_SMOOTHER_*  (JACOBI)                                   */
    unsigned nu1, nu2, nuCoarse;   /* 0: keep the hierarchy's; SPMV_AMG_NO_SWEEPS: none       */
    double   eigRatio;      /* lambda_min = lambda_max / eigRatio (10); must be > 1            */
    double   lambdaScale;   /* lambda_max_l = lambdaScale * rho_l (1.0)                        */
} spmvAmgSmootherOpts;
typedef struct { int kind; unsigned nu1, nu2, nuCoarse; double rho, lambdaMax, lambdaMin;
                 unsigned nCoef; const double* dCoef; } spmvAmgSmootherInfo;
int spmvHipAmgSetSmoother(spmat* dM, spmat* dA, const spmvAmgSmootherOpts* opts);
int spmvHipAmgSmoother(spmat* dM, unsigned level, spmvAmgSmootherInfo* info);
typedef struct {            /* 0 = the built-in default */
    int      order;         /* SPMV_COLOUR_NATURAL (default) or SPMV_COLOUR_HASH                     */
    uint32_t seed;          /* of the HASH keys                                                      */
    double   omega;         /* relaxation (1.0); must be finite and > 0                              */
    int      oneWay;        /* 0: forward before the correction, backward after it (symmetric);      */
                            /* 1: forward everywhere                                                 */
    unsigned levels;        /* Gauss-Seidel on levels l < levels, damped Jacobi (V above) below; 0: all */
    unsigned nu1, nu2, nuCoarse;   /* as in spmvAmgSmootherOpts: 0 keeps, SPMV_AMG_NO_SWEEPS none, <= SPMV_AMG_MAX_DEGREE */
} spmvAmgGsOpts;
typedef struct { int active; unsigned colours; ulong maxColourRows, longRows; int small; double omega; int order; uint32_t seed;
                 int oneWay; const uint32_t* dPerm; const uint32_t* dColourPtr; } spmvAmgGsInfo;
int spmvHipAmgSetGaussSeidel(spmat* dM, spmat* dA, const spmvAmgGsOpts* opts);
int spmvHipAmgGaussSeidel(spmat* dM, unsigned level, spmvAmgGsInfo* info);
typedef struct { unsigned width; ulong bytes; } spmvAmgBlockInfo;
int spmvHipAmgSetBlockWidth(spmat* dM, spmat* dA, unsigned width);
int spmvHipAmgBlock(spmat* dM, spmvAmgBlockInfo* info);
/* The hierarchy stored in single precision (SPMV_STORAGE_* and spmvHipValuesF32 are declared above and
 * below).  spmvHipAmgSetStorage(dM, dA, SPMV_STORAGE_F32) builds the single-precision value form on every matrix a product of
 * the cycle streams: dA itself (level 0 is the caller's handle: it gets the form as by spmvHipValuesF32(dA, 1)), every A_l
 * below it, every R_l and every P_l; all of them or none.  Every A_l z, R_l d and P_l e of spmvHipAmgApply, of
 * spmvHipAmgApplyBlock and of a hierarchy as dM is then the f32 product (hipSpMVRowsCSRf32 / hipSpMMRowsCSRf32: serial order on
 * the values rounded through float, arithmetic in double), the fused z + P e its f32 instance with the bits of the unfused
 * pair; the plain hierarchy's gather correction has no values.  dinv_l, rho_l and the Chebyshev tables stay what the double
 * values give.  For the plain, smoothed and strength hierarchies, the Jacobi and the Chebyshev smoother.  The cycle is still
 * one fixed linear operator, symmetric if it was.  spmvHipAmgRefresh keeps the setting: the forms follow the levels' new
 * values.  SPMV_STORAGE_F64, the state after a setup, releases the forms (dA's only if this call built it).  Synchronous,
 * allocates 4 B per entry of those matrices; idempotent.  hipFreeSpmat(dM) of an F32 hierarchy frees the forms of its own
 * levels with them; the form on dA is dA's and stays until spmvHipValuesF32(dA, 0) or hipFreeSpmat(dA).  While a hierarchy of
 * dA is stored in F32, releasing dA's form makes its cycles refuse until the form is built again.
 * Refused with a message, the hierarchy left as it was: what spmvHipAmgRefresh refuses; a storage that is neither constant;
 * F32 on a hierarchy with a Gauss-Seidel level (its sweeps read the double values in kernels of their own) -- and
 * spmvHipAmgSetGaussSeidel on an F32 hierarchy; a failed allocation (what the call built is released).
 * spmvHipAmgStorage: the setting, the number of levels, and the bytes of the f32 forms over all levels (0 in F64). */
typedef struct { int storage; unsigned levels; ulong f32Bytes; } spmvAmgStorageInfo;
int spmvHipAmgSetStorage(spmat* dM, spmat* dA, int storage);
int spmvHipAmgStorage(spmat* dM, spmvAmgStorageInfo* info);
int spmvHipAmgApplyBlock(spmat* dM, spmat* dA, unsigned k, const double* dR, size_t ldr, int rLayout,
                         double* dZ, size_t ldz, int zLayout);
/* Release the device arrays behind a handle (cudaUtils.h:70-78). */
int hipFreeSpmat(spmat* dMat);

/* Adopt arrays that are ALREADY on the device in device format (u32 columns,
 * u32 or u64 row pointers) -- used by the on-device synthetic generator and by
 * callers that assemble matrices on the GPU.  The handle takes ownership of
 * nothing: the caller frees the arrays after hipFreeSpmat(). `irpBytes` is 4 or 8.
 * `hIRP` is the same row-pointer array on the host (needed for the row-block
 * analysis); it may be NULL, in which case it is downloaded.
 * VALUES ARE A SNAPSHOT.  `dAS` is read at adopt (unit detection: spmvHipSetUnitValues) and copied into every private
 * format built later (two-phase, stripes, SELL), which keep their copy.  `dAS` must therefore be complete on the device
 * before this call (it runs on the null stream).  Rewriting `dAS` afterwards is NOT seen -- y then mixes old and new
 * values -- until the caller says so with spmvHipValuesChanged(), or writes new values through spmvHipUpdateValues().
 * hipSpILU0CSR on an adopted handle overwrites `dAS` in place with the factors. */
int spmvHipAdoptCSR(spmat* dMat, ulong M, ulong N, ulong NZ,
                    const void* dIRP, int irpBytes, const uint32_t* dJA,
                    const double* dAS, const void* hIRP);

/* ------------------------------------------------------ new values, same pattern */
/* For iterative callers (Newton steps, time steps, parameter sweeps) whose values change while the sparsity pattern stays:
 * what a handle costs to make -- upload, row-block analysis, the measured kernel selection of hipSpMVRowsCSR /
 * hipSpMVWarpPerRowCSR, the private formats -- depends on the pattern only, and is kept.
 *
 * spmvHipUpdateValues: new values for `dMat`.  `AS` has the handle's value layout and is read from the host
 * (asOnDevice = 0) or the device (asOnDevice = 1):
 *   spMatCpyCSR / spmvHipAdoptCSR handle   NZ values in CSR order; copied into the handle's AS -- for an adopted handle
 *                                          that is the caller's own dAS, which it handed over at adopt
 *   spMatCpyELL / spMatCpyELLTransposed    the host ELL value array in the layout of the upload (row-major rows x slots,
 *                                          or the transposed slots x rows); copied into the pitched device array
 *   spmvHipCsrToEll handle                 REFUSED: it keeps no link to its source (update the source, convert again)
 * spmvHipValuesChanged: the handle's own value array was rewritten on the device by the caller (an adopted dAS, or the
 *   array published in dMat->AS); the formats and the unit detection re-read it.  Same refusals.
 *
 * KEPT across an update: IRP, JA, RL, the row blocks; every built format's index arrays in both of its forms; the form
 * preferences (spmvHipBuild*Opt); the kernel selections (spmvHipAutoChoice[Rows]) -- a launch after the update runs the
 * same kernel as before, so the reduction-order name gives the same bits for the same values; every device address.
 * REFRESHED: AS, the unit detection (spmvHipUnitValue; off with spmvHipSetUnitValues(0)), and the value array of every
 * format that has been built, in every form.  Formats not built stay unbuilt.  The two-phase and the stripes format keep
 * a map from their storage order to CSR order for this (4 B per entry and form, reported in spmvHip*Bytes, freed with the
 * format); it is built at the format's FIRST update, never before -- a handle that is never updated costs nothing more.
 * NaN and Inf are values like any other.
 * Unit transitions ("all stored values equal", spmvHipSetUnitValues): unit -> unit with another value changes only the
 * value the kernels take from a register; non-unit -> unit switches to the unit kernels (y unchanged: c * x rounds as
 * AS[j] * x does); unit -> non-unit rebuilds, with its recorded options, a stripes format that was built without a value
 * array, and forgets both kernel selections (their measurements counted the bytes of the unit kernels): the next call of
 * each name measures again.
 * spmvUpdateInfo (spmvHipLastUpdateInfo, the handle's last update): inPlace = 1 when every launch captured before the
 * update (a HIP graph) computes with the new values as it stands: same kernels, same arguments, refreshed arrays at their
 * old addresses -- 0 after a unit transition other than non-unit -> unit, or when a format was rebuilt (rebuilt = 1: its
 * addresses changed).  mapsBuilt = value maps built by this call, mapMs their build time, ms the whole call (host wall
 * time), unitBefore / unitAfter the unit detection around it.
 * Streams: everything is enqueued on the library stream (spmvHipSetStream) and the call returns with the values in place,
 * like the other synchronous calls.  The unit detection reads one word back (and a first build of a map, or a rebuild,
 * synchronises the device).  A device `AS` -- and for ValuesChanged the handle's own array -- must be complete on that
 * stream before the call.  Launches already enqueued on other streams that read this handle must be finished by the caller.
 * Refused with a message and EXIT_FAILURE, the handle left as it was: NULL handle or AS, something that is not a live
 * handle (never made, or freed), a derived ELL handle. */
typedef struct {
    int    inPlace, rebuilt, mapsBuilt, unitBefore, unitAfter;
    double ms, mapMs;
} spmvUpdateInfo;
int spmvHipUpdateValues(spmat* dMat, const double* AS, int asOnDevice);
int spmvHipValuesChanged(spmat* dMat);
int spmvHipLastUpdateInfo(spmat* dMat, spmvUpdateInfo* info);

/* --------------------------------------------------------------- SpMV on GPU */
/* y = A x with A, x, y resident on the device.  (mat, x, CONFIG by value, y):
 * the parameter list of the reference's SPMV_CUDA typedef (SpMV.h:119-120). */
typedef int (SPMV_HIP)(spmat*, double*, CONFIG, double*);
typedef int (*SPMV_HIP_INTERF)(spmat*, double*, CONFIG, double*);

SPMV_HIP hipSpMVRowsCSR;                  /* <- cudaSpMVRowsCSR                  SpMV_CUDA.cu:33-49   */
SPMV_HIP hipSpMVWarpPerRowCSR;            /* <- cudaSpMVWarpPerRowCSR            SpMV_CUDA.cu:52-73   */
SPMV_HIP hipSpMVRowsELL;                  /* <- cudaSpMVRowsELL (transposed)     SpMV_CUDA.cu:79-96   */
SPMV_HIP hipSpMVRowsELLNNTransposed;      /* <- cudaSpMVRowsELLNNTransposed      SpMV_CUDA.cu:99-115  */
SPMV_HIP hipSpMVWarpsPerRowELLNTrasposed; /* <- cudaSpMVWarpsPerRowELLNTrasposed SpMV_CUDA.cu:116-135 */

/* --------------------------------------------------------- blocks of vectors */
#define SPMV_DENSE_ROW_MAJOR 0   /* element (i, c) at P[i*ld + c], ld >= k          */
#define SPMV_DENSE_COL_MAJOR 1   /* element (i, c) at P[c*ld + i], ld >= rows of P  */
/* Y = A X for k >= 1 columns.  X is N x k and Y is M x k, both on the device; each has its own layout and leading
 * dimension.  Column c of Y has the bits of sgemvSerial(A, X[:, c]): every row's products are rounded and added in the
 * handle's stored entry order, exactly as the oracle walks it.  For block solvers (block CG / GMRES, LOBPCG), several
 * right-hand sides, probing: one call instead of k calls of hipSpMVRowsCSR, which stream the matrix k times (DESIGN.md
 * section 15).
 * Handles: CSR handles from spMatCpyCSR and spmvHipAdoptCSR, 4- or 8-byte row pointers.  ELL handles (spmvHipCsrToEll's
 *   included) are refused.
 * Order: the stored order, not the sorted one -- the bits hold for unsorted rows and for repeated columns too, and do not
 *   rest on the LDS atomic order (spmvHipProbeLdsAtomicOrder).  An empty row gives +0.0 in every column; NaN and Inf
 *   propagate as in the oracle.  Elements of Y outside the M x k block (the ld padding) are never written.
 * Width: any k >= 1.  The columns are taken in panels of at most 16 and the matrix is streamed once per panel (k = 17 is
 *   two panels: twice the matrix).  k = 1 with unit strides runs the LDS-stream kernel of hipSpMVRowsCSR (variant 1): the
 *   bits of hipSpMVRowsCSR.  Row-major X and Y are the fast layout; column-major X gathers one line per element.
 * Values are read at every call: AS and the unit detection (spmvHipUnitValue: the value then comes from a register, Y
 *   unchanged), so the next call after spmvHipUpdateValues / spmvHipValuesChanged uses the new values.
 * Launch: as the SpMV launchers -- spmvHipSetSync(1) waits, then sets spmvHipLastKernelSeconds (all panels) and
 *   spmvHipLastLaunch (one panel's shape); spmvHipSetSync(0) only enqueues on the library stream.  No device allocation,
 *   no format: the call can be captured into a HIP graph.
 * Refused with a message and EXIT_FAILURE, Y untouched: NULL pointers or a handle that is not live, an ELL handle,
 *   k = 0, an unknown layout, ld too small for its layout, X and Y address ranges that overlap (checked on the host). */
int hipSpMMRowsCSR(spmat* dMat, unsigned k, const double* dX, size_t ldx, int xLayout,
                   double* dY, size_t ldy, int yLayout);

/* ------------------------------------------- single-precision value storage */
/* A CSR handle can keep a second copy of its values in single precision, 4 B per entry beside the 8 B of AS, for the
 * products whose values need not be exact (a preconditioner's factors): a product then streams 8 instead of 12 bytes per
 * entry.  Only the STORAGE is single precision.  x, y, every product, every sum and their order stay what they are; the
 * value is widened -- exactly -- when it is loaded.  DESIGN.md section 41.  The form is this loop over the NZ entries,
 *     for p = 0 .. NZ-1:  AS32[p] = (float)AS[p]                          -- IEEE round to nearest, ties to even
 * with single-precision subnormals kept (nothing is flushed that is representable); a magnitude at or above
 * (2 - 2^-24) * 2^127 becomes +-Inf and Inf stays Inf; a NaN stays a NaN (payload unspecified); the sign of a zero, and of
 * a value that rounds to zero, is kept.  With A~_p = (double)AS32[p], an f32 product is sgemvSerial on A~ bit for bit
 * (the serial-order names) or its sums in another order (the reduction-order name), as the f64 names are on A.
 * A unit handle (every stored value the same double, spmvHipUnitValue) gets no array: its register value is rounded the
 * same way on the host and the unit kernels serve it.
 * spmvHipValuesF32(dMat, on): on != 0 builds the form and keeps it (one elementwise pass; one device allocation of
 *   4 NZ bytes rounded up to 16, plus 32 for the pass's counters; a unit handle: none), on == 0 releases it at once: the
 *   array is freed, spmvHipValuesF32Info reports zeros and -1 again, the f32 products refuse the handle until it is built
 *   again, and that build starts at refreshes = 0.  Idempotent,
 *   synchronous on the library stream.  The form belongs to the handle like the two-phase, stripes and SELL formats, is
 *   freed with it, and FOLLOWS the values: after spmvHipUpdateValues / spmvHipValuesChanged, every refresh of a derived
 *   handle, spmvHipCooAssembleRefresh and hipSpILU0CSR it holds the roundings of the new values at the same address.  A unit -> non-unit update
 *   allocates the array, the reverse frees it; if that allocation is refused the update fails with a message, the handle
 *   keeps its new double values and stays usable, and the form is not built (build it again).
 *   No f64 call changes what it returns, which kernel it picks or what it allocates, built or not.
 *   Accepted: CSR matrix handles of any origin (uploaded, adopted with 4- or 8-byte row pointers, derived).  Refused with
 *   a message: NULL, a handle that is not live, an ELL handle, a multigrid hierarchy, a handle with entries but no value
 *   array, and a live sharded matrix (the void* of spmvHipShardCSR handed in as the handle: recognised and refused before it is
 *   read; its per-device handles are private to the shard and have no such form).
 * spmvHipValuesF32Info: built, unit (built without an array), bytes (the allocation), refreshes (value updates followed
 *   since the build), and for the build or the last refresh: inexact = entries p, not NaN, with (double)AS32[p] != AS[p]
 *   (overflowed and flushed entries are among them); overflowed = finite AS[p] with infinite AS32[p]; flushed = nonzero
 *   AS[p] with zero AS32[p]; firstOverflow = the smallest such CSR position, -1 for none.  The counts are integer atomics
 *   after a wavefront count, so they do not depend on the order of anything.  Not built: zeros and -1.
 * The products.  hipSpMVRowsCSRf32 (serial order) and hipSpMVWarpPerRowCSRf32 (any reduction order) have the signatures,
 *   the synchronisation and the timing of their f64 twins; CONFIG is not looked at.  spmvHipEnqueueRowsF32 is the
 *   enqueue-only serial-order form on an explicit stream.  hipSpMMRowsCSRf32 has the signature, layouts, panel rule and
 *   refusals of hipSpMMRowsCSR, and every column of Y has the bits of hipSpMVRowsCSRf32.  All four are served by the
 *   LDS-stream kernel (hipSpMVRowsCSR's variant 1) and its block form: there is no timed selection and no f32 form of the
 *   other formats.  They never allocate -- capturable, enqueue-only under spmvHipSetSync(0) -- and refuse, with a message
 *   that names spmvHipValuesF32, a handle whose form is not built. */
typedef struct {
    int   built;            /* the form exists                                                          */
    int   unit;             /* ... without an array: the handle is a unit handle                        */
    ulong bytes;            /* of its device allocation                                                 */
    ulong refreshes;        /* value updates it has followed since it was built                         */
    ulong inexact;          /* of the build or the last refresh: entries that changed under rounding    */
    ulong overflowed;       /* ... finite entries that became +-Inf                                     */
    ulong flushed;          /* ... nonzero entries that became +-0                                      */
    long  firstOverflow;    /* ... the first overflowed CSR position, -1: none                          */
} spmvF32Info;
int spmvHipValuesF32(spmat* dMat, int on);
int spmvHipValuesF32Info(spmat* dMat, spmvF32Info* info);
SPMV_HIP hipSpMVRowsCSRf32;
SPMV_HIP hipSpMVWarpPerRowCSRf32;
int spmvHipEnqueueRowsF32(spmat* dMat, double* dX, double* dY, void* stream);
int hipSpMMRowsCSRf32(spmat* dMat, unsigned k, const double* dX, size_t ldx, int xLayout,
                      double* dY, size_t ldy, int yLayout);

/* Column-sliced two-phase SpMV for matrices whose x gather misses the caches
 * (DESIGN.md section 7): the GPU counterpart of the reference's 2-D decomposed
 * CPU variants spmvTilesCSR / spmvTilesAllocdCSR (src/SpMV_CSR_OMP.c:101-226:
 * column partitions, partial results, final reduction).  The slice-major copy
 * of the matrix (+12 B/nnz of device memory per matrix, plus ONE product
 * workspace of 8 B/nnz of the largest matrix, shared by all matrices of the
 * device and used in stream order) is built on the device at the first call, or
 * explicitly with spmvHipBuildTiles.  Row sums are added in
 * arrival order (LDS atomics): equal to the oracle to rounding, not bitwise -- unless the
 * deterministic form was asked for with spmvHipBuildTilesOpt (serial order, the oracle's bits;
 * +4 B/nnz).  The launcher runs the form last asked for (default: arrival order); a handle can
 * hold both. */
SPMV_HIP hipSpMVTilesCSR;
int    spmvHipBuildTiles(spmat* dMat);
size_t spmvHipTilesBytes(spmat* dMat);

/* One-pass SpMV with y bins in LDS and x served by the XCD's L2: rows are cut into
 * bins of <= 20 000 consecutive rows with equal entry counts, a workgroup owns a bin, and inside a bin the
 * entries are stored in COLUMN order, so that the workgroups resident on one XCD sweep x together and gather
 * from its L2.  12 B/nnz of streaming (fp64 value + {17-bit column offset, 15-bit local row}) and no second
 * pass -- the intent of cudaSpMVWarpPerRowCSR (src/SpMV_CUDA.cu:52-73: coalesced AS/JA, gathered x, on-chip
 * reduction) with the reduction in LDS accumulators.  The copy of the matrix (+12 B/nnz of device memory)
 * is built on the device at the first call or with spmvHipBuildStripes.  Pays off while x (N * 8 B) is small
 * against the entry stream; very wide matrices are the two-phase kernel's.  Row sums are added in arrival
 * order (LDS atomics): equal to the oracle to rounding, not bitwise -- unless a deterministic form was asked for with
 * spmvHipBuildStripesOpt (below).  The launcher runs the form last asked for (default: arrival order). */
SPMV_HIP hipSpMVStripesCSR;
int    spmvHipBuildStripes(spmat* dMat);
size_t spmvHipStripesBytes(spmat* dMat);
/* shape of the built format (zeros before the build): bins, rows of the highest bin, 1 if the 14 B/nnz
 * encoding with 32-bit columns had to be used, device time of the one-time build in ms */
int    spmvHipStripesShape(spmat* dMat, unsigned* nBins, unsigned* rowsPerBin, int* wide, double* buildMs);
/* Build options of the stripes format (all zero / -1 = automatic).  Arguments of the build, not process state:
 * spmvHipBuildStripesOpt(dMat, &opts) builds -- or REbuilds -- the format of this handle with them.
 *   rowsPerBin     0 or 1..20000: upper bound of the rows of a bin (y of a bin lives in LDS).
 *   grid           0 or 1..CUs of the device: persistent workgroups that walk the bins (the bin count is made a
 *                  multiple of it); fewer than the CU count leaves CUs to a kernel running beside this one.
 *   spread         -1 or 0..1024: 1/1024ths of a bin over which the column sweeps of one XCD's workgroups start
 *                  (default 6; ignored by the deterministic form).
 *   wide           1: force the 14 B/nnz encoding with 32-bit columns; 0 / -1: only when a step spans >= 2^17 columns.
 *   deterministic  1 or 2: a row's products are added in ascending column order, so the result is the same bits in every run,
 *                  on any number of row shards, and -- the products being rounded before they are added -- the bits of the
 *                  serial oracle (sgemvSerial, src/SpMV_CSR_OMP.c:229-250) when the columns of every row ascend, as the
 *                  reference's loader guarantees (src/lib/parser.c:195-202).  The build does not check that: on a row whose
 *                  columns do not ascend both forms add the row's products stably sorted by column (equal columns in stored
 *                  order), which is not the oracle's order there.  1 = "owner wavefronts": every row is added by
 *                  ONE wavefront (local row mod 4 owns it) walking its own column-ordered sub-stream -- a layout of its own;
 *                  nearly free on matrices with column locality, 1.5-2x on uniformly spread columns (a gather covers
 *                  neighbours of a quarter of the bin's entries).  2 = "ordered tickets": the layout and the shared stream
 *                  of the arrival-order kernel (options 0 and 2 build the same format), but the batches add in ticket order,
 *                  handed over through an LDS word: 1.2x on uniformly spread columns, 1.5x where many lanes of an
 *                  instruction meet in a row (narrow bands).  hipSpMVRowsCSR's default measures both. */
typedef struct { unsigned rowsPerBin; unsigned grid; int spread; int wide; int deterministic; } spmvStripesOpts;
int spmvHipBuildStripesOpt(spmat* dMat, const spmvStripesOpts* opts);
typedef struct {
    unsigned nBins, rowsPerBin, grid, spread;
    int      wide, deterministic;
    double   buildMs;          /* device time of the one-time build */
    size_t   bytes;            /* device memory of the format */
} spmvStripesInfo;
int spmvHipStripesInfo(spmat* dMat, spmvStripesInfo* info);   /* zeros when the format has not been built */

/* The fastest CSR launcher for THIS matrix, chosen by measurement at the first call for a handle (the reference's
 * callers choose a kernel by name -- CUDA_CSR_ROWS_WARP, ... -- src/main.cu:103-139; which of this library's kernels
 * wins depends on where x lives relative to the caches, DESIGN.md sections 4, 7, 8).  Candidates: hipSpMVWarpPerRowCSR
 * always; from 2^18 entries on hipSpMVTilesCSR and, while x (N * 8 B) fits the 256 MiB Infinity Cache,
 * hipSpMVStripesCSR.  The first call runs every eligible candidate on the caller's x (one launch that also builds its
 * format + 3 timed ones, a single one if it takes more than 2 ms; each leaves the complete y), keeps the fastest and frees the private formats of the others;
 * it synchronises the stream even after spmvHipSetSync(0).  Later calls go straight to the chosen launcher.
 * spmvHipAutoChoice: its name (NULL before the first call) and, if msPerCandidate != NULL, the three measured times in
 * ms in the order above (0 = not eligible / not tried; room for FOUR doubles, the fourth stays 0).  Arrival-order sums
 * when a format kernel wins. */
SPMV_HIP hipSpMVAutoCSR;
const char* spmvHipAutoChoice(spmat* dMat, double* msPerCandidate);
/* The same report for the selection hipSpMVRowsCSR (variant 2) makes among the SERIAL-ORDER kernels: "hipSpMVRowsCSR" (the
 * LDS-stream kernel, one thread per row), "hipSpMVTilesCSR(deterministic)", "hipSpMVStripesCSR(owner wavefronts)",
 * "hipSpMVStripesCSR(ordered tickets)"; FOUR times in that order.  Whichever is chosen, y is the bits of sgemvSerial. */
const char* spmvHipAutoChoiceRows(spmat* dMat, double* msPerCandidate);

/* SELL-C-sigma (C = 64 rows per slice = one wavefront, rows sorted by length inside 16 Ki-row
 * windows, column-major inside a slice) built on the device from an uploaded CSR handle at the
 * first call: the ELL-family kernel for matrices whose longest row makes plain ELL impossible
 * (the reference's loader refuses them, src/lib/parser.c:223-232).  One lane per
 * row, ascending-j order: bit-identical to the serial oracle for rows up to 256 entries;
 * longer rows are summed by a whole workgroup (shuffle tree). */
SPMV_HIP hipSpMVRowsSELL;
int    spmvHipBuildSell(spmat* dMat);
size_t spmvHipSellBytes(spmat* dMat);

/* Enqueue-only form of the two CSR launchers on an explicit stream (no timing
 * bracket, no synchronisation): warpPerRow = 0 -> hipSpMVRowsCSR semantics,
 * != 0 -> hipSpMVWarpPerRowCSR.  The current device must be the matrix'. */
int spmvHipEnqueueCSR(spmat* dMat, int warpPerRow, double* dX, double* dY, void* stream);
/* The same for the launcher hipSpMVAutoCSR / hipSpMVWarpPerRowCSR (variant 2) chose for this handle; the FIRST call for a
 * handle measures the candidates on `stream` and synchronises it (later calls only enqueue). */
int spmvHipEnqueueAuto(spmat* dMat, double* dX, double* dY, void* stream);
/* ... and for the launcher hipSpMVRowsCSR (variant 2) chose: serial-order sums, y bit-identical to sgemvSerial. */
int spmvHipEnqueueAutoRows(spmat* dMat, double* dX, double* dY, void* stream);

/* 1 when this device adds the lanes of one LDS atomic instruction that meet in an address in ascending lane order and runs a
 * wavefront's LDS operations in issue order -- measured by a probe kernel against host sums, cached; 0 otherwise, -1 before
 * spmvHipInit.  The deterministic forms of the two-phase and the stripes kernel give the serial oracle's bits BECAUSE of
 * this (it is observed behaviour of gfx950, not an ISA promise): hipSpMVRowsCSR's serial-order selection offers them only
 * where the probe returns 1 and otherwise stays with the kernel that sums a row in one thread. */
int spmvHipProbeLdsAtomicOrder(void);

/* Kernel variants behind each launcher (for A/B measurement; default = best):
 *   hipSpMVRowsCSR        0 = one thread walks its row in global memory: the plain restatement of
 *                             cudaSpMVRowsCSR (uncoalesced; 5-6x slower, profiles/r01_variants.md)
 *                         1 = LDS-stream kernel: coalesced span load, products parked in LDS, one
 *                             thread sums its row in ascending-j order (bit-identical to the serial oracle)
 *                         2 = (default) the fastest of this library's SERIAL-ORDER kernels for THIS matrix -- variant 1
 *                             and the deterministic forms of the two-phase and the stripes kernel (spmvTilesOpts /
 *                             spmvStripesOpts .deterministic) -- chosen by measurement at the first call for a handle,
 *                             like variant 2 of hipSpMVWarpPerRowCSR below (same first-call cost, same +12 B/nnz for
 *                             the winner's copy of the matrix; matrices below 2^18 entries go straight to variant 1).
 *                             Every candidate adds a row's products in ascending column order with the product rounded
 *                             first, so y is the bits of sgemvSerial whichever is chosen (for rows whose columns ascend,
 *                             which the reference's loader guarantees, src/lib/parser.c:195-202).  Reached by the
 *                             reference's names SpmvCUDA_CSRFuncs[0], CUDA_CSR_ROWS, spmvHipRowsCSR.
 *   hipSpMVWarpPerRowCSR  0 = one wavefront per row, __shfl_down tree (the reference kernel's intent, for
 *                             every row)
 *                         1 = LDS-stream kernel with the LDS segmented reduction for short rows and
 *                             wavefront-/workgroup-per-row sums for long ones
 *                         2 = (default) the fastest of this library's reduction-order kernels for THIS matrix --
 *                             variant 1, hipSpMVTilesCSR, hipSpMVStripesCSR -- chosen exactly as hipSpMVAutoCSR does:
 *                             the FIRST call for a handle runs the eligible candidates on the caller's x (each leaves
 *                             the complete y; matrices below 2^18 entries go straight to variant 1), keeps the
 *                             fastest and frees the others' formats.  Cost of that first call: a handful of SpMVs
 *                             plus the format builds (c3: ~0.15 s; c5: ~1-2 s, mostly allocation) and it synchronises
 *                             the stream; afterwards +12 B/nnz of device memory for the winner's copy of the matrix
 *                             (+ the shared 8 B/nnz product workspace when the two-phase kernel wins).  This is what
 *                             the reference's names reach: SpmvCUDA_CSRFuncs[SpmvCUDA_CSRFuncs_WarpPerRowIdx],
 *                             CUDA_CSR_ROWS_WARP, spmvHipWarpPerRowCSR (src/include/SpMV.h:130-134).  A caller that
 *                             wants the one-kernel behaviour of round 1/2 sets variant 1 (CLI: SPMV_VARIANT=1).
 *   hipSpMVRowsELLNNTransposed  0 = one thread walks its row of the row-major matrix in global memory: the plain
 *                             restatement of cudaSpMVRowsELLNNTransposed (a lane's loads lie a pitch apart: uncoalesced by
 *                             construction, the reference's slowest kernel); also what runs when CONFIG.blockSize is given
 *                         1 = (default) the same sums -- one thread adds its row's cells in ascending slot order, bit for
 *                             bit -- fed from a coalesced span parked in LDS (rows of up to 2048 slots; longer: variant 0)
 *   hipSpTRSVCSR              T, 0..65536: the row threshold of the single-workgroup runs for triangles analysed after
 *                             the call (default 256; 0 = a launch per level).  x does not change by a bit.
 *   hipSpILU0CSR              8, 16 or 64: the lanes that factor one row (default 16).  AS does not change by a bit.
 *   hipSpCGCSR, hipSpBiCGStabCSR  K, 1..4096: iterations enqueued per read-back of the solver's device state
 *                             (default 16).  x does not change by a bit.
 *   hipSpCGBlockCSR, hipSpBiCGStabBlockCSR  K, 1..4096: iterations enqueued per read-back of the block's all-stopped
 *                             word (default 16).  No column changes by a bit.
 *   hipSpGMRESCSR             0 or 1: 1 folds the first CGS2 update into the partials of the second projection
 *                             (default 0).  x does not change by a bit.
 *   spmvHipColourCSR          K, 1..4096: rounds enqueued per read-back of the colouring's device state (default 16,
 *                             unmeasured).  No colour changes.
 *   spmvHipRcmCSR             T, 0 and up, clamped to 1024: levels of at most T vertices are expanded one after the other
 *                             inside one launch of one workgroup (default 1024; 0 = never: every level with an edge takes
 *                             a launch over its frontier and a read-back).  No word of dPerm changes.
 *   spmvHipAmgApply           n, 0..4096: hierarchies set up by spmvHipAmgSetupSmoothed AFTER the call correct in one fused
 *                             kernel on every level whose prolongator has no row longer than n entries (default 0 = never
 *                             fused, an SpMV and an add: the faster form on the 5 M-row Laplacian, DESIGN.md section 28;
 *                             64 is the long-row convention).  z does not change by a bit.
 *   spmvHipAmgSetGaussSeidel  n, 0..65536: spmvHipAmgSetGaussSeidel calls made AFTER the call sweep a level of at most n rows
 *                             in one launch of one workgroup (default 1024, unmeasured; 0 = never: a launch per colour).
 *                             z does not change by a bit.
 *   spmvHipAmgGaussSeidel     g, one of 0, 1, 4, 8, 16, 32, 64: the lanes that take one row in the sweeps of
 *                             spmvHipAmgSetGaussSeidel calls made AFTER the call (default 0 = per level, the largest power of
 *                             two from 4 to 64 that the mean row fills; 1 = a lane per row, a wavefront above 64 entries;
 *                             DESIGN.md section 32 has both measured).  z does not change by a bit.
 * Returns EXIT_FAILURE for an unknown (launcher, variant). */
int spmvHipSetVariant(const char* launcher, int variant);
/* Use the RL array for ELL early exit (1, default when RL was uploaded) or walk
 * all MAX_ROW_NZ slots like the reference's cudaSpMVRowsELL (0). */
int spmvHipSetEllRowLens(int useRowLens);
/* Matrices whose stored values are ALL THE SAME double -- MatrixMarket `pattern` files, which the loader fills with 1.0
 * (src/lib/parser.c:59-61): every graph of the DIMACS10 collection, among them asia_osm and channel-500x100x100-b050 of
 * the reference's report -- are recognised when a CSR matrix is uploaded or adopted (one pass over the values).  The CSR
 * kernels (LDS-stream, stripes, two-phase) then take the value from a register instead of streaming 8 B per entry: 4 B/nnz
 * of matrix traffic instead of 12.  y does not change by a bit (c * x[j] rounds as AS[j] * x[j] does).  Compared as bit
 * patterns.  spmvHipSetUnitValues(0) turns the recognition off for later uploads (A/B); spmvHipUnitValue: 1 and the value,
 * 0, or -1 for a bad handle. */
int spmvHipSetUnitValues(int on);
int spmvHipUnitValue(spmat* dMat, double* value);

/* SPMV_INTERF-compatible wrappers (host vectors in/out, matrix uploaded and
 * cached on first use, keyed by the host spmat address) so the GPU path can sit
 * in SpmvCSRFuncs[]-style tables next to the OpenMP variants (SpMV.h:146-159).
 * The cache entry also remembers the shape and the IRP/JA/AS/RL pointers it was
 * uploaded from and is re-uploaded when any of them differs; changing the values
 * INSIDE the same arrays is not seen: call spmvHipDropCache() before a cached
 * host matrix is modified or freed. */
int spmvHipRowsCSR(spmat* mat, double* x, CONFIG* cfg, double* y);
int spmvHipWarpPerRowCSR(spmat* mat, double* x, CONFIG* cfg, double* y);
int spmvHipRowsELL(spmat* mat, double* x, CONFIG* cfg, double* y);
int spmvHipWarpsPerRowELL(spmat* mat, double* x, CONFIG* cfg, double* y);
int spmvHipDropCache(void);

/* ------------------------------------------------------- events (measurement) */
int spmvHipEventCreate(void** ev);
int spmvHipEventDestroy(void* ev);
int spmvHipEventRecord(void* ev);                 /* on the stream set above */
int spmvHipEventElapsedMs(void* evStart, void* evStop, float* ms);  /* syncs on evStop */

/* ------------------------------------------------------------------ sharding */
/* nnz-balanced contiguous row blocks: bounds[p]..bounds[p+1] are the rows of
 * part p (bounds has nParts+1 entries).  IRP is a host row-pointer array. */
int spmvHipPartitionRows(const ulong* IRP, ulong M, int nParts, ulong* bounds);
/* Extract rows [r0,r1) of a host CSR matrix as a new host CSR (local IRP
 * rebased to 0, global column ids kept).  Free with freeSpmat(). */
spmat* spmvHipRowBlockCSR(const spmat* host, ulong r0, ulong r1);
/* After an all-gather of equally padded row blocks (dYPad = nParts blocks of
 * maxRows doubles, block p holding rows bounds[p]..bounds[p+1]) copy the rows
 * back to back into dY -- nParts device-to-device copies on the library stream.  A block longer than maxRows is
 * refused before anything is copied: dY is left as it was. */
int spmvHipCompactRows(double* dY, const double* dYPad, const ulong* bounds, int nParts, ulong maxRows);
/* Single-process multi-device path (C drivers): shard, upload one block per
 * device, replicate x, run `mode` on every device concurrently, gather y with
 * an RCCL all-gather over xGMI.  bench.py uses one process per GPU instead and
 * calls the single-device entry points + torch.distributed (RCCL). */
int spmvHipShardCSR(spmat* host, int nDev, void** shardHandle);
/* ... with every device's rows cut into `groups` consecutive row groups (0 = automatic: 2 when nDev > 1): the
 * all-gather of group g runs on its own stream while group g+1 is computed. */
int spmvHipShardCSRGroups(spmat* host, int nDev, int groups, void** shardHandle);
/* mode 0: the kernel hipSpMVRowsCSR runs (variant 2: the fastest serial-order kernel per block; y bit-identical to the
 * 1-GPU result and to sgemvSerial); mode != 0: that of hipSpMVWarpPerRowCSR (variant 2: the fastest reduction-order kernel
 * per block).  Either selection is made by an untimed pass at the first call with that mode.  kernelSec = kernels of all row groups, slowest device; gatherSec = what the exchange adds after overlap. */
int spmvHipSpMVSharded(void* shardHandle, const double* hX, int mode, double* hY,
                       double* kernelSec, double* gatherSec);
int spmvHipShardFree(void* shardHandle);
/* New values for a sharded matrix of the same pattern: `hAS` (host) holds the WHOLE matrix's NZ values in CSR order; every
 * row block gets its slice and is updated on its own device (spmvHipUpdateValues, on that device's compute stream), the
 * per-block kernel selections stay.  Refused: NULL, a handle that is not a live shard (freed with spmvHipShardFree). */
int spmvHipShardUpdateValues(void* shardHandle, const double* hAS);

/* ------------------------------------ peer windows: one process per GPU, xGMI */
/* bench.py's layout (one process per GPU) exchanges y with RCCL by default.  xGMI
 * is a point-to-point mesh, so the same exchange can also be written as every rank
 * PUSHING its rows straight into the other ranks' copies of y.  A "window" is a
 * device allocation other processes of the node can map: its 64-byte handle is
 * plain data the caller ships to them however it likes (bench.py: torch.distributed
 * all_gather_object).  New functionality -- the reference is single-GPU. */
#define SPMV_IPC_HANDLE_BYTES 64
#define SPMV_MAX_PEERS 15
int spmvHipWindowCreate(size_t bytes, void** dBase, unsigned char handle[SPMV_IPC_HANDLE_BYTES]);
int spmvHipWindowFree(void* dBase);
/* Map a window exported by ANOTHER process whose GPU is device `ownerDev` in this
 * process' numbering, readable/writable from the current device (peer access is
 * enabled when the devices differ).  Close before the owner frees it. */
int spmvHipWindowOpen(const unsigned char handle[SPMV_IPC_HANDLE_BYTES], int ownerDev, void** dPeer);
int spmvHipWindowClose(void* dPeer);
/* Copy bytes [offset, offset+bytes) of the own buffer `dSrcBase` to the same offset
 * of every peer mapping, one copy engine stream per peer, all ordered after what is
 * enqueued on the library stream so far; returns at once.  spmvHipPeerPushJoin()
 * makes the library stream wait for every push issued before it. */
int spmvHipPeerPush(const void* dSrcBase, size_t offset, size_t bytes, int nPeers, void* const* dPeerBases);
int spmvHipPeerPushJoin(void);

/* The two phases of hipSpMVTilesCSR as separate launches, for callers that overlap
 * the exchange of y with its production: Expand = phase 1 over the whole matrix;
 * Reduce = phase 2 for the bins [binBegin, binEnd) -- rows [binBegin*rowsPerBin,
 * min(binEnd*rowsPerBin, M)) -- stored to dY and, when nExtra > 0, also to the
 * nExtra further vectors dExtra[k] with the same row indexing (peer mappings: the
 * all-gather fused into the kernel as direct xGMI stores).  Enqueue-only when
 * spmvHipSetSync(0).  spmvHipTilesShape builds the format if needed. */
int spmvHipTilesShape(spmat* dMat, unsigned* nBins, unsigned* rowsPerBin);
/* Build options of the two-phase format (all zero / -1 = automatic).  They are arguments of the build, not
 * process state: spmvHipBuildTilesOpt(dMat, &opts) builds -- or REbuilds -- the format of this handle with them.
 *   rowsPerBin  0 or 64..20000.  Phase 2 finishes its bins in rounds of one workgroup per CU, and rows can only
 *               leave for the other ranks when their bin is finished: when the exchange is the longer part of a
 *               step, smaller bins (more rounds) let it start earlier, at the price of shorter tiles (N = 8 shard
 *               of c5: 1.19 ms automatic, 1.26 ms with half-size bins, 1.43 ms with quarter-size ones).
 *   taper       1: one round (one bin per CU) of quarter-height bins first and last, full-height bins between --
 *               the first round sets when rows start to travel, the last what is still to be sent when phase 2
 *               ends.  rowsPerBin of spmvHipTilesShape is then the height of the HIGHEST bin; spmvHipTilesBinRow
 *               gives the first row of any bin (bin == nBins: the row count).
 *   ntStore     1 / 0: phase 1 stores the products non-temporally / with the default policy; -1: by size
 *               (products that fit the 256 MiB Infinity Cache are kept there).
 *   chunk       entries per phase-1 work item, 0 or 4096..2^24.
 *   deterministic  1: every row is added by ONE wavefront in ascending column order (a bin is four sub-bins, each walked by
 *               one wavefront), so y is the same bits in every run and on any number of row shards, and -- products being
 *               rounded before they are added -- the bits of the serial oracle when the columns of every row ascend.
 *               The build does not check that.  Precisely, a row is added in its stored order stably sorted by SLICE
 *               (column >> 14, 16 Ki columns): the same as ascending columns on sorted rows, but on a row whose columns
 *               do not ascend the entries of one slice keep their stored order (the stripes forms sort them by column).
 *               Costs time: four wavefronts per CU instead of sixteen, tiles a quarter as long.  No
 *               tapered bins in this form. */
typedef struct { unsigned rowsPerBin; int taper; int ntStore; unsigned chunk; int deterministic; } spmvTilesOpts;
int spmvHipBuildTilesOpt(spmat* dMat, const spmvTilesOpts* opts);
typedef struct {
    unsigned nBins, rowsPerBin, nSlices;
    int      taper, ntStore;
    unsigned chunk;
    double   buildMs;          /* wall time of the one-time build, allocations included */
    size_t   bytes;            /* device memory of the format (the shared product workspace not included) */
    double   allocMs;          /* the part of buildMs the host spent in hipMalloc: format, product workspace, temporaries */
    size_t   tempBytes;        /* peak of the temporaries of the build (12 B per entry + the tile tables; freed when it returns) */
    int      deterministic;
} spmvTilesInfo;
int spmvHipTilesInfo(spmat* dMat, spmvTilesInfo* info);   /* zeros when the format has not been built */
int spmvHipTilesBinRow(spmat* dMat, unsigned bin, ulong* firstRow);
int hipSpMVTilesExpand(spmat* dMat, double* dX);
int hipSpMVTilesReduce(spmat* dMat, unsigned binBegin, unsigned binEnd, double* dY, int nExtra, double* const* dExtra);
/* Phase 2 over all bins with a PUSH KERNEL beside it (own high-priority stream, no LDS, a few wavefronts per CU):
 * every reduction workgroup sets a per-bin flag when its rows of y are stored (agent-scope release), the push
 * kernel copies each flagged bin to the nExtra destinations.  The reduction never waits for a link and the links
 * work from the first finished bin on.  With spmvHipSetSync(0) the library stream does NOT wait for the push
 * kernel (the next row group's phase 1 may run while these rows still travel): spmvHipTilesPushJoin() makes it
 * wait for every push kernel enqueued so far; in synchronous mode the call returns with everything delivered.
 * A flag that does not arrive within ~2 s makes the push kernel give up (spmvHipTilesPushFailed() == 1, y
 * incomplete) rather than hang. */
int hipSpMVTilesReducePush(spmat* dMat, double* dY, int nExtra, double* const* dExtra);
int spmvHipTilesPushJoin(void);
int spmvHipTilesPushFailed(spmat* dMat);

/* ------------------------------------------------- synthetic matrices on device */
/* Fill JA/AS of a CSR whose row pointers are given (device arrays, device
 * format), for global rows [rowOffset, rowOffset+M): DESIGN.md "Synthetic
 * inputs".  band == 0: columns stratified-uniform over [0,N); band > 0: columns
 * stratified over [r-band, r+band] clipped to [0,N). */
int spmvHipSynthFillCSR(ulong M, ulong N, ulong rowOffset, const void* dIRP, int irpBytes,
                        uint32_t* dJA, double* dAS, uint64_t seedStruct, uint64_t seedVal,
                        ulong band);
/* (the dense vector x is generated on the host -- it needs sin(), whose last
 * bit differs between libm and the device -- and uploaded with spmvHipVecUp) */

#ifdef __cplusplus
}
#endif
#endif /* SPMV_HIP_H */
