"""Python mirror of the C driver surface (include/spmvHip.h, include/SpMV.h).

Same names, argument meaning and error behaviour (0 = EXIT_SUCCESS, 1 =
EXIT_FAILURE, diagnostics on stderr) as the C entry points, which in turn mirror
the reference (src/include/SpMV.h:119-142, src/include/cudaUtils.h:60-78).
Everything numeric happens in libspmvhip.so; numpy is only used to marshal host
arrays.  The library is REQUIRED: there is no fallback implementation.
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np

from .ctypes_defs import CONFIG, POISON_NAN, SPMAT_TAG_ELL_TRANSPOSED, spmat, spmvDim3

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPMV_LIB") or os.path.join(_HERE, "lib", "libspmvhip.so")      # SPMV_LIB: tuning builds only
HOSTLIB_PATH = os.path.join(_HERE, "lib", "libspmvhost.so")


class SpmvHipError(RuntimeError):
    pass


def _load(path):
    if not os.path.exists(path):
        raise SpmvHipError(
            f"{path} is missing: build it with `make lib host` (or __graft_entry__.build()). "
            "This package has no CPU fallback.")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


lib = _load(LIB_PATH)
hostlib = _load(HOSTLIB_PATH)

_vp, _sz, _u64, _i = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int
_SPMV_ARGS = [C.POINTER(spmat), _vp, CONFIG, _vp]
_sigs = {
    "spmvHipInit": ([_i, _sz, _sz], _i), "spmvHipFinalize": ([], _i), "spmvHipDeviceCount": ([], _i),
    "spmvHipSetStream": ([_vp], _i), "spmvHipSetSync": ([_i], _i), "spmvHipProbeLdsAtomicOrder": ([], _i),
    "spmvHipLastKernelSeconds": ([], C.c_double),
    "spmvHipLastLaunch": ([C.POINTER(spmvDim3), C.POINTER(spmvDim3)], _i),
    "spmvHipDeviceSynchronize": ([], _i),
    "spmvHipVecAlloc": ([C.POINTER(_vp), _sz], _i), "spmvHipVecFree": ([_vp], _i),
    "spmvHipVecUp": ([_vp, _vp, _sz], _i), "spmvHipVecDown": ([_vp, _vp, _sz], _i),
    "spmvHipVecFill": ([_vp, _sz, _u64], _i),
    "spmvHipMalloc": ([C.POINTER(_vp), _sz], _i), "spmvHipFree": ([_vp], _i),
    "spmvHipMemcpyUp": ([_vp, _vp, _sz], _i), "spmvHipMemcpyDown": ([_vp, _vp, _sz], _i),
    "spmvHipAllocRefuse": ([C.c_long, _i], _i), "spmvHipAllocStats": ([_vp], _i),
    "spMatCpyCSR": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "spMatCpyELL": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "spMatCpyELLTransposed": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "hipFreeSpmat": ([C.POINTER(spmat)], _i),
    "spmvHipCsrToEll": ([C.POINTER(spmat), _i, C.POINTER(spmat)], _i),
    "spmvHipAdoptCSR": ([C.POINTER(spmat), C.c_ulong, C.c_ulong, C.c_ulong, _vp, _i, _vp, _vp, _vp], _i),
    "hipSpMVRowsCSR": (_SPMV_ARGS, _i), "hipSpMVWarpPerRowCSR": (_SPMV_ARGS, _i),
    "hipSpMVRowsSELL": (_SPMV_ARGS, _i), "spmvHipBuildSell": ([C.POINTER(spmat)], _i),
    "spmvHipSellBytes": ([C.POINTER(spmat)], _sz),
    "hipSpMVTilesCSR": (_SPMV_ARGS, _i), "spmvHipBuildTiles": ([C.POINTER(spmat)], _i),
    "spmvHipTilesBytes": ([C.POINTER(spmat)], _sz),
    "hipSpMVStripesCSR": (_SPMV_ARGS, _i), "spmvHipBuildStripes": ([C.POINTER(spmat)], _i),
    "hipSpMVAutoCSR": (_SPMV_ARGS, _i), "spmvHipAutoChoice": ([C.POINTER(spmat), C.POINTER(C.c_double)], C.c_char_p),
    "spmvHipStripesBytes": ([C.POINTER(spmat)], _sz),
    "spmvHipStripesShape": ([C.POINTER(spmat), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(_i), C.POINTER(C.c_double)], _i),
    "spmvHipEnqueueCSR": ([C.POINTER(spmat), _i, _vp, _vp, _vp], _i),
    "spmvHipEnqueueAuto": ([C.POINTER(spmat), _vp, _vp, _vp], _i),
    "spmvHipEnqueueAutoRows": ([C.POINTER(spmat), _vp, _vp, _vp], _i),
    "spmvHipAutoChoiceRows": ([C.POINTER(spmat), C.POINTER(C.c_double)], C.c_char_p),
    "spmvHipBuildStripesOpt": ([C.POINTER(spmat), _vp], _i), "spmvHipStripesInfo": ([C.POINTER(spmat), _vp], _i),
    "spmvHipShardCSR": ([C.POINTER(spmat), _i, C.POINTER(_vp)], _i),
    "spmvHipShardCSRGroups": ([C.POINTER(spmat), _i, _i, C.POINTER(_vp)], _i),
    "spmvHipSpMVSharded": ([_vp, _vp, _i, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double)], _i),
    "spmvHipShardFree": ([_vp], _i),
    "hipSpMVRowsELL": (_SPMV_ARGS, _i), "hipSpMVRowsELLNNTransposed": (_SPMV_ARGS, _i),
    "hipSpMVWarpsPerRowELLNTrasposed": (_SPMV_ARGS, _i),
    "spmvHipSetVariant": ([C.c_char_p, _i], _i), "spmvHipSetEllRowLens": ([_i], _i),
    "spmvHipSetUnitValues": ([_i], _i), "spmvHipUnitValue": ([C.POINTER(spmat), C.POINTER(C.c_double)], _i),
    "spmvHipRowsCSR": ([C.POINTER(spmat), _vp, C.POINTER(CONFIG), _vp], _i),
    "spmvHipWarpPerRowCSR": ([C.POINTER(spmat), _vp, C.POINTER(CONFIG), _vp], _i),
    "spmvHipRowsELL": ([C.POINTER(spmat), _vp, C.POINTER(CONFIG), _vp], _i),
    "spmvHipWarpsPerRowELL": ([C.POINTER(spmat), _vp, C.POINTER(CONFIG), _vp], _i),
    "spmvHipDropCache": ([], _i),
    "spmvHipEventCreate": ([C.POINTER(_vp)], _i), "spmvHipEventDestroy": ([_vp], _i),
    "spmvHipEventRecord": ([_vp], _i), "spmvHipEventElapsedMs": ([_vp, _vp, C.POINTER(C.c_float)], _i),
    "spmvHipPartitionRows": ([_vp, C.c_ulong, _i, _vp], _i),
    "spmvHipRowBlockCSR": ([C.POINTER(spmat), C.c_ulong, C.c_ulong], C.POINTER(spmat)),
    "spmvHipSynthFillCSR": ([C.c_ulong, C.c_ulong, C.c_ulong, _vp, _i, _vp, _vp, _u64, _u64, C.c_ulong], _i),
    "spmvHipCompactRows": ([_vp, _vp, _vp, _i, C.c_ulong], _i),
    "spmvHipWindowCreate": ([_sz, C.POINTER(_vp), _vp], _i), "spmvHipWindowFree": ([_vp], _i),
    "spmvHipWindowOpen": ([_vp, _i, C.POINTER(_vp)], _i), "spmvHipWindowClose": ([_vp], _i),
    "spmvHipPeerPush": ([_vp, _sz, _sz, _i, _vp], _i), "spmvHipPeerPushJoin": ([], _i),
    "spmvHipTilesShape": ([C.POINTER(spmat), C.POINTER(C.c_uint), C.POINTER(C.c_uint)], _i),
    "hipSpMVTilesExpand": ([C.POINTER(spmat), _vp], _i),
    "hipSpMVTilesReduce": ([C.POINTER(spmat), C.c_uint, C.c_uint, _vp, _i, _vp], _i),
    "hipSpMVTilesReducePush": ([C.POINTER(spmat), _vp, _i, _vp], _i), "spmvHipTilesPushFailed": ([C.POINTER(spmat)], _i),
    "spmvHipTilesPushJoin": ([], _i),
    "spmvHipBuildTilesOpt": ([C.POINTER(spmat), _vp], _i), "spmvHipTilesInfo": ([C.POINTER(spmat), _vp], _i),
    "spmvHipTilesBinRow": ([C.POINTER(spmat), C.c_uint, C.POINTER(C.c_ulong)], _i),
    "spmvHipUpdateValues": ([C.POINTER(spmat), _vp, _i], _i), "spmvHipValuesChanged": ([C.POINTER(spmat)], _i),
    "spmvHipLastUpdateInfo": ([C.POINTER(spmat), _vp], _i), "spmvHipShardUpdateValues": ([_vp, _vp], _i),
    "hipSpMMRowsCSR": ([C.POINTER(spmat), C.c_uint, _vp, _sz, _i, _vp, _sz, _i], _i),
    "spmvHipCsrTranspose": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "spmvHipTransposeRefresh": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "spmvHipTriAnalyse": ([C.POINTER(spmat), _i], _i),
    "hipSpTRSVCSR": ([C.POINTER(spmat), _i, _i, _vp, _vp], _i),
    "spmvHipTriInfo": ([C.POINTER(spmat), _i, _vp], _i),
    "hipSpTRSMCSR": ([C.POINTER(spmat), _i, _i, C.c_uint, _vp, _sz, _i, _vp, _sz, _i], _i),
    "spmvHipTriSweepsPrepare": ([C.POINTER(spmat), C.c_uint], _i),
    "hipSpTRSVSweepsCSR": ([C.POINTER(spmat), _i, _i, C.c_uint, _vp, _vp], _i),
    "hipSpTRSMSweepsCSR": ([C.POINTER(spmat), _i, _i, C.c_uint, C.c_uint, _vp, _sz, _i, _vp, _sz, _i], _i),
    "spmvHipTriSetApply": ([C.POINTER(spmat), _i, C.c_uint, C.c_uint, C.c_uint], _i),
    "spmvHipTriSweepsInfo": ([C.POINTER(spmat), _vp], _i),
    "hipSpILU0CSR": ([C.POINTER(spmat)], _i),
    "spmvHipIlu0Info": ([C.POINTER(spmat), _vp], _i),
    "spmvHipFsaiSetup": ([C.POINTER(spmat), C.POINTER(spmat), _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipFsaiRefresh": ([C.POINTER(spmat), C.POINTER(spmat), _vp], _i),
    "spmvHipFsaiApply": ([C.POINTER(spmat), _vp, _vp], _i),
    "spmvHipFsaiTranspose": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "spmvHipFsaiInfo": ([C.POINTER(spmat), _vp], _i),
    "spmvHipFsaiSetStorage": ([C.POINTER(spmat), _i], _i), "spmvHipFsaiStorage": ([C.POINTER(spmat), C.POINTER(_i)], _i),
    "spmvHipValuesF32": ([C.POINTER(spmat), _i], _i), "spmvHipValuesF32Info": ([C.POINTER(spmat), _vp], _i),
    "hipSpMVRowsCSRf32": (_SPMV_ARGS, _i), "hipSpMVWarpPerRowCSRf32": (_SPMV_ARGS, _i),
    "spmvHipEnqueueRowsF32": ([C.POINTER(spmat), _vp, _vp, _vp], _i),
    "hipSpMMRowsCSRf32": ([C.POINTER(spmat), C.c_uint, _vp, _sz, _i, _vp, _sz, _i], _i),
    "spmvHipDot": ([_sz, _vp, _vp, _vp], _i),
    "hipSpCGCSR": ([C.POINTER(spmat), C.POINTER(spmat), _vp, _vp, _vp, _vp], _i),
    "hipSpBiCGStabCSR": ([C.POINTER(spmat), C.POINTER(spmat), _vp, _vp, _vp, _vp], _i),
    "spmvHipMultiDot": ([_sz, C.c_uint, _vp, _sz, _vp, _vp], _i),
    "spmvHipBlockDot": ([_sz, C.c_uint, _vp, _sz, _i, _vp, _sz, _i, _vp], _i),
    "hipSpCGBlockCSR": ([C.POINTER(spmat), C.POINTER(spmat), C.c_uint, _vp, _sz, _i, _vp, _sz, _i, _vp, _vp, _vp], _i),
    "hipSpBiCGStabBlockCSR": ([C.POINTER(spmat), C.POINTER(spmat), C.c_uint, _vp, _sz, _i, _vp, _sz, _i, _vp, _vp, _vp], _i),
    "hipSpGMRESCSR": ([C.POINTER(spmat), C.POINTER(spmat), _vp, _vp, _vp, _vp], _i),
    "spmvHipBlockCombine": ([_sz, C.c_uint, C.c_uint, _vp, _sz, _vp, _sz, _vp, _sz], _i),
    "hipSpLanczosCSR": ([C.POINTER(spmat), _vp, _vp, _vp, _sz, _vp, _vp, _vp], _i),
    "spmvHipBlockResidual": ([_sz, C.c_uint, C.c_uint, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp], _i),
    "hipSpDavidsonCSR": ([C.POINTER(spmat), C.POINTER(spmat), _vp, _vp, _vp, _sz, _vp, _vp, _vp], _i),
    "spmvHipColourCSR": ([C.POINTER(spmat), _vp, _vp, _vp, _vp], _i),
    "spmvHipCsrPermute": ([C.POINTER(spmat), _vp, C.POINTER(spmat)], _i),
    "spmvHipPermuteRefresh": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "spmvHipVecPermute": ([_sz, _vp, _vp, _vp, _i], _i),
    "spmvHipRcmCSR": ([C.POINTER(spmat), _vp, _vp, _vp], _i),
    "spmvHipSpGEMM": ([C.POINTER(spmat), C.POINTER(spmat), _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipSpGEMMRefresh": ([C.POINTER(spmat), C.POINTER(spmat), C.POINTER(spmat), _vp], _i),
    "spmvHipCsrAdd": ([C.c_double, C.POINTER(spmat), C.c_double, C.POINTER(spmat), _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipCsrAddRefresh": ([C.POINTER(spmat), C.c_double, C.POINTER(spmat), C.c_double, C.POINTER(spmat), _vp], _i),
    "spmvHipCsrFilter": ([C.POINTER(spmat), _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipCsrFilterRefresh": ([C.POINTER(spmat), C.POINTER(spmat), _vp], _i),
    "spmvHipCooAssemble": ([C.c_ulong, C.c_ulong, C.c_ulong, _vp, _vp, _vp, _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipCooAssembleRefresh": ([C.POINTER(spmat), C.c_ulong, _vp, _vp], _i),
    "spmvHipCsrToCoo": ([C.POINTER(spmat), _vp, _vp, _vp], _i),
    "spmvHipAggregateCSR": ([C.POINTER(spmat), _vp, _vp, _vp], _i),
    "spmvHipAmgSetup": ([C.POINTER(spmat), _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipAmgRefresh": ([C.POINTER(spmat), C.POINTER(spmat)], _i),
    "spmvHipAmgApply": ([C.POINTER(spmat), C.POINTER(spmat), _vp, _vp], _i),
    "spmvHipAmgInfo": ([C.POINTER(spmat), _vp], _i),
    "spmvHipAmgLevel": ([C.POINTER(spmat), C.c_uint, C.POINTER(spmat), C.POINTER(_vp), C.POINTER(_vp)], _i),
    "spmvHipAmgSetupSmoothed": ([C.POINTER(spmat), _vp, _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipAmgProlongator": ([C.POINTER(spmat), C.c_uint, C.POINTER(spmat), C.POINTER(spmat), C.POINTER(C.c_double)], _i),
    "spmvHipAmgSetupStrength": ([C.POINTER(spmat), _vp, _vp, _vp, C.POINTER(spmat), _vp], _i),
    "spmvHipAmgStrength": ([C.POINTER(spmat), C.c_uint, C.POINTER(spmat), C.POINTER(C.c_double)], _i),
    "spmvHipAmgSetSmoother": ([C.POINTER(spmat), C.POINTER(spmat), _vp], _i),
    "spmvHipAmgSmoother": ([C.POINTER(spmat), C.c_uint, _vp], _i),
    "spmvHipAmgSetGaussSeidel": ([C.POINTER(spmat), C.POINTER(spmat), _vp], _i),
    "spmvHipAmgGaussSeidel": ([C.POINTER(spmat), C.c_uint, _vp], _i),
    "spmvHipAmgSetBlockWidth": ([C.POINTER(spmat), C.POINTER(spmat), C.c_uint], _i),
    "spmvHipAmgBlock": ([C.POINTER(spmat), _vp], _i),
    "spmvHipAmgSetStorage": ([C.POINTER(spmat), C.POINTER(spmat), _i], _i), "spmvHipAmgStorage": ([C.POINTER(spmat), _vp], _i),
    "spmvHipAmgApplyBlock": ([C.POINTER(spmat), C.POINTER(spmat), C.c_uint, _vp, _sz, _i, _vp, _sz, _i], _i),
}
SPMV_DENSE_ROW_MAJOR, SPMV_DENSE_COL_MAJOR = 0, 1          # include/spmvHip.h: layouts of hipSpMMRowsCSR's X and Y
SPMV_TRI_LOWER, SPMV_TRI_UPPER = 0, 1                      # include/spmvHip.h: hipSpTRSVCSR's uplo ...
SPMV_DIAG_STORED, SPMV_DIAG_UNIT = 0, 1                    # ... and diag
SPMV_TRI_APPLY_EXACT, SPMV_TRI_APPLY_SWEEPS = 0, 1         # include/spmvHip.h: spmvHipTriSetApply's mode
SPMV_TRI_SWEEPS_MAX = 4096                                 # ... and the most sweeps of one solve
SPMV_EIG_LARGEST, SPMV_EIG_SMALLEST = 0, 1                 # include/spmvHip.h: spmvLanczosOpts.which
EIG_WHICH = {"LA": SPMV_EIG_LARGEST, "SA": SPMV_EIG_SMALLEST}      # DeviceMatrix.eigsh's `which`
SPMV_STORAGE_F64, SPMV_STORAGE_F32 = 0, 1                  # include/spmvHip.h: spmvHipFsaiSetStorage's storage
STORAGES = {"f64": SPMV_STORAGE_F64, "f32": SPMV_STORAGE_F32}


def _storage(s, who):
    if s not in STORAGES:
        raise SpmvHipError(f"{who}: storage {s!r} is neither 'f64' nor 'f32'")
    return STORAGES[s]


class spmvTilesOpts(C.Structure):
    """include/spmvHip.h `spmvTilesOpts` (0 / 0 / -1 / 0 = automatic)."""
    _fields_ = [("rowsPerBin", C.c_uint), ("taper", _i), ("ntStore", _i), ("chunk", C.c_uint), ("deterministic", _i)]

    def __init__(self, rowsPerBin=0, taper=0, ntStore=-1, chunk=0, deterministic=0):
        super().__init__(rowsPerBin, taper, ntStore, chunk, deterministic)


class spmvTilesInfo(C.Structure):
    _fields_ = [("nBins", C.c_uint), ("rowsPerBin", C.c_uint), ("nSlices", C.c_uint), ("taper", _i), ("ntStore", _i),
                ("chunk", C.c_uint), ("buildMs", C.c_double), ("bytes", _sz), ("allocMs", C.c_double), ("tempBytes", _sz),
                ("deterministic", _i)]


class spmvStripesOpts(C.Structure):
    """include/spmvHip.h `spmvStripesOpts` (0 / 0 / -1 / -1 / 0 = automatic)."""
    _fields_ = [("rowsPerBin", C.c_uint), ("grid", C.c_uint), ("spread", _i), ("wide", _i), ("deterministic", _i)]

    def __init__(self, rowsPerBin=0, grid=0, spread=-1, wide=-1, deterministic=0):
        super().__init__(rowsPerBin, grid, spread, wide, deterministic)


class spmvStripesInfo(C.Structure):
    _fields_ = [("nBins", C.c_uint), ("rowsPerBin", C.c_uint), ("grid", C.c_uint), ("spread", C.c_uint), ("wide", _i),
                ("deterministic", _i), ("buildMs", C.c_double), ("bytes", _sz)]


class spmvUpdateInfo(C.Structure):
    """include/spmvHip.h `spmvUpdateInfo`: what the last value update of a handle did."""
    _fields_ = [("inPlace", _i), ("rebuilt", _i), ("mapsBuilt", _i), ("unitBefore", _i), ("unitAfter", _i),
                ("ms", C.c_double), ("mapMs", C.c_double)]


class spmvTriInfo(C.Structure):
    """include/spmvHip.h `spmvTriInfo`: the level-set schedule of one triangle (all zeros: not analysed)."""
    _fields_ = [("levels", C.c_ulong), ("maxLevelRows", C.c_ulong), ("launches", C.c_ulong), ("fusedLevels", C.c_ulong),
                ("longRows", C.c_ulong), ("firstBadDiag", C.c_long), ("analyses", _i), ("analysisMs", C.c_double),
                ("bytes", _sz)]


class spmvTriSweepsInfo(C.Structure):
    """include/spmvHip.h `spmvTriSweepsInfo`: the plan of the triangular solves by Jacobi sweeps (all zeros: no plan)."""
    _fields_ = [("mode", _i), ("lowerSweeps", C.c_uint), ("upperSweeps", C.c_uint), ("width", C.c_uint),
                ("solveLaunches", C.c_ulong), ("applyLaunches", C.c_ulong), ("firstBadDiag", C.c_long), ("sorted", _i),
                ("prepares", _i), ("bytes", _sz), ("diagPos", _vp), ("workspace", _vp)]


class spmvIluInfo(C.Structure):
    """include/spmvHip.h `spmvIluInfo`: what the last ILU(0) factorisation of a handle did."""
    _fields_ = [("zeroPivot", C.c_long), ("firstBadRow", C.c_long), ("levels", C.c_ulong), ("launches", C.c_ulong),
                ("longRows", C.c_ulong), ("factorisations", _i), ("ms", C.c_double)]


SPMV_FSAI_MAX_ROW = 64                                     # include/spmvHip.h: the longest row of an approximate-inverse factor


class spmvF32Info(C.Structure):
    """include/spmvHip.h `spmvF32Info`: the single-precision value form of a handle and what its last rounding pass did."""
    _fields_ = [("built", _i), ("unit", _i), ("bytes", C.c_ulong), ("refreshes", C.c_ulong), ("inexact", C.c_ulong),
                ("overflowed", C.c_ulong), ("flushed", C.c_ulong), ("firstOverflow", C.c_long)]


class spmvFsaiOpts(C.Structure):
    """include/spmvHip.h `spmvFsaiOpts`: the lanes that compute one row of G (0: the built-in choice; 4, 16 or 64)."""
    _fields_ = [("lanesPerRow", C.c_uint)]


class spmvFsaiInfo(C.Structure):
    """include/spmvHip.h `spmvFsaiInfo`: what the setup or the last refresh of an approximate-inverse factor did."""
    _fields_ = [("nnz", C.c_ulong), ("maxRow", C.c_ulong), ("badRows", C.c_ulong), ("firstBadRow", C.c_long),
                ("launches", C.c_ulong), ("setups", C.c_ulong), ("ms", C.c_double)]


class spmvKrylovOpts(C.Structure):
    """include/spmvHip.h `spmvKrylovOpts`: tolerance, iteration cap, optional host history (maxIter + 1 doubles)."""
    _fields_ = [("tol", C.c_double), ("maxIter", C.c_ulong), ("history", C.POINTER(C.c_double))]


class spmvGmresOpts(C.Structure):
    """include/spmvHip.h `spmvGmresOpts`: tolerance, cap on the inner iterations, restart length (1 .. 64), optional host
    history (maxIter + 1 doubles)."""
    _fields_ = [("tol", C.c_double), ("maxIter", C.c_ulong), ("restart", C.c_uint), ("history", C.POINTER(C.c_double))]


class spmvLanczosOpts(C.Structure):
    """include/spmvHip.h `spmvLanczosOpts`: eigenpairs wanted, Lanczos vectors of a cycle, the end of the spectrum,
    tolerance, cap on the products A v, columns a restart keeps (0: the default)."""
    _fields_ = [("nev", C.c_uint), ("ncv", C.c_uint), ("which", _i), ("tol", C.c_double), ("maxIter", C.c_ulong),
                ("keep", C.c_uint)]


class spmvLanczosInfo(C.Structure):
    """include/spmvHip.h `spmvLanczosInfo`: what a hipSpLanczosCSR call did."""
    _fields_ = [("status", _i), ("found", C.c_uint), ("iterations", C.c_ulong), ("cycles", C.c_ulong), ("launches", C.c_ulong),
                ("hostChecks", C.c_ulong), ("scale", C.c_double), ("sweepsMax", C.c_uint), ("ms", C.c_double), ("jacobiMs", C.c_double)]


class spmvDavidsonOpts(C.Structure):
    """include/spmvHip.h `spmvDavidsonOpts`: eigenpairs wanted (at most 16), columns of the basis at most, the end of the
    spectrum, tolerance, cap on the products A v, columns a restart keeps (0: the default)."""
    _fields_ = [("nev", C.c_uint), ("ncv", C.c_uint), ("which", _i), ("tol", C.c_double), ("maxIter", C.c_ulong),
                ("keep", C.c_uint)]


class spmvDavidsonInfo(C.Structure):
    """include/spmvHip.h `spmvDavidsonInfo`: what a hipSpDavidsonCSR call did."""
    _fields_ = [("status", _i), ("found", C.c_uint), ("iterations", C.c_ulong), ("restarts", C.c_ulong), ("precondApplies", C.c_ulong),
                ("launches", C.c_ulong), ("hostChecks", C.c_ulong), ("scale", C.c_double), ("sweepsMax", C.c_uint), ("ms", C.c_double),
                ("jacobiMs", C.c_double)]


class spmvKrylovInfo(C.Structure):
    """include/spmvHip.h `spmvKrylovInfo`: what a hipSpCGCSR / hipSpBiCGStabCSR call did."""
    _fields_ = [("status", _i), ("iterations", C.c_ulong), ("rr", C.c_double), ("bb", C.c_double), ("launches", C.c_ulong),
                ("hostChecks", C.c_ulong), ("ms", C.c_double)]


class spmvKrylovColumn(C.Structure):
    """include/spmvHip.h `spmvKrylovColumn`: what one column of a hipSpCGBlockCSR / hipSpBiCGStabBlockCSR call did."""
    _fields_ = [("status", _i), ("iterations", C.c_ulong), ("rr", C.c_double), ("bb", C.c_double)]


class spmvColourOpts(C.Structure):
    """include/spmvHip.h `spmvColourOpts`: the order of the colouring and the seed of the HASH keys."""
    _fields_ = [("order", _i), ("seed", C.c_uint32)]


class spmvColourInfo(C.Structure):
    """include/spmvHip.h `spmvColourInfo`: what a spmvHipColourCSR call did."""
    _fields_ = [("colours", C.c_ulong), ("rounds", C.c_ulong), ("hostChecks", C.c_ulong), ("maxColourRows", C.c_ulong),
                ("longRows", C.c_ulong), ("symmetric", _i), ("ms", C.c_double)]


class spmvRcmOpts(C.Structure):
    """include/spmvHip.h `spmvRcmOpts`: the start rule, the passes of the start search (0: 8), forward != 0 for the unreversed order."""
    _fields_ = [("start", _i), ("maxPasses", C.c_uint), ("forward", _i)]


class spmvRcmInfo(C.Structure):
    """include/spmvHip.h `spmvRcmInfo`: what a spmvHipRcmCSR call did."""
    _fields_ = [("components", C.c_ulong), ("levels", C.c_ulong), ("startBfs", C.c_ulong), ("maxFrontier", C.c_ulong),
                ("longRows", C.c_ulong), ("symmetric", _i), ("bandwidthBefore", C.c_ulong), ("bandwidthAfter", C.c_ulong),
                ("launches", C.c_ulong), ("hostChecks", C.c_ulong), ("ms", C.c_double)]


class spmvSpgemmOpts(C.Structure):
    """include/spmvHip.h `spmvSpgemmOpts`: the class limits of spmvHipSpGEMM (0 = the built-in default; they only lower)."""
    _fields_ = [("waveMaxProducts", C.c_ulong), ("groupMaxProducts", C.c_ulong), ("sortBudgetBytes", C.c_ulong)]


class spmvSpgemmInfo(C.Structure):
    """include/spmvHip.h `spmvSpgemmInfo`: what a spmvHipSpGEMM / spmvHipSpGEMMRefresh call did."""
    _fields_ = [("products", C.c_ulong), ("nnzC", C.c_ulong), ("maxRowProducts", C.c_ulong), ("maxRowNnz", C.c_ulong),
                ("rowsWave", C.c_ulong), ("rowsGroup", C.c_ulong), ("rowsSorted", C.c_ulong), ("sortBatches", C.c_ulong),
                ("tempBytes", C.c_ulong), ("symbolicMs", C.c_double), ("numericMs", C.c_double), ("ms", C.c_double)]


class spmvAddOpts(C.Structure):
    """include/spmvHip.h `spmvAddOpts`: the class limits of spmvHipCsrAdd (0 = the built-in default; they only lower)."""
    _fields_ = [("laneMaxTerms", C.c_ulong), ("waveMaxTerms", C.c_ulong), ("sortBudgetBytes", C.c_ulong), ("allSorted", _i)]


class spmvAddInfo(C.Structure):
    """include/spmvHip.h `spmvAddInfo`: what a spmvHipCsrAdd / spmvHipCsrAddRefresh call did."""
    _fields_ = [("terms", C.c_ulong), ("nnzC", C.c_ulong), ("maxRowTerms", C.c_ulong), ("maxRowNnz", C.c_ulong),
                ("rowsLane", C.c_ulong), ("rowsWave", C.c_ulong), ("rowsSorted", C.c_ulong), ("sortBatches", C.c_ulong),
                ("tempBytes", C.c_ulong), ("symbolicMs", C.c_double), ("numericMs", C.c_double), ("ms", C.c_double)]


SPMV_FILTER_BAND, SPMV_FILTER_ABS, SPMV_FILTER_STRENGTH = 0, 1, 2
FILTER_MODES = {"band": SPMV_FILTER_BAND, "abs": SPMV_FILTER_ABS, "strength": SPMV_FILTER_STRENGTH}
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


class spmvFilterOpts(C.Structure):
    """include/spmvHip.h `spmvFilterOpts`: the predicate of spmvHipCsrFilter (lo / hi: INT64_MIN / INT64_MAX are the open ends)."""
    _fields_ = [("mode", _i), ("lo", C.c_int64), ("hi", C.c_int64), ("theta", C.c_double), ("lump", _i)]


class spmvFilterInfo(C.Structure):
    """include/spmvHip.h `spmvFilterInfo`: what a spmvHipCsrFilter / spmvHipCsrFilterRefresh call did."""
    _fields_ = [("nnzA", C.c_ulong), ("nnzC", C.c_ulong), ("maxRowNnz", C.c_ulong), ("lumpedRows", C.c_ulong),
                ("tempBytes", C.c_ulong), ("ms", C.c_double)]


SPMV_COO_SKIP, SPMV_COO_SUM, SPMV_COO_LAST = 0xFFFFFFFF, 0, 1
COO_DUPLICATES = {"sum": SPMV_COO_SUM, "last": SPMV_COO_LAST}


class spmvCooOpts(C.Structure):
    """include/spmvHip.h `spmvCooOpts`: what spmvHipCooAssemble does with duplicates, and whether it keeps the map of a refresh."""
    _fields_ = [("duplicates", _i), ("keepMap", _i)]


class spmvCooInfo(C.Structure):
    """include/spmvHip.h `spmvCooInfo`: what a spmvHipCooAssemble / spmvHipCooAssembleRefresh call did."""
    _fields_ = [("nEntries", C.c_ulong), ("skipped", C.c_ulong), ("nnzC", C.c_ulong), ("duplicates", C.c_ulong),
                ("maxRun", C.c_ulong), ("maxRowNnz", C.c_ulong), ("tempBytes", C.c_ulong), ("ms", C.c_double)]


SPMV_AMG_MAX_LEVELS, SPMV_AMG_NO_SWEEPS = 16, 0xFFFFFFFF


class spmvAggOpts(C.Structure):
    """include/spmvHip.h `spmvAggOpts`: the seed of the keys."""
    _fields_ = [("seed", C.c_uint32)]


class spmvAggInfo(C.Structure):
    """include/spmvHip.h `spmvAggInfo`: what a spmvHipAggregateCSR call did."""
    _fields_ = [("aggregates", C.c_ulong), ("rounds", C.c_ulong), ("hostChecks", C.c_ulong), ("longRows", C.c_ulong),
                ("symmetric", _i), ("maxAggRows", C.c_ulong), ("minAggRows", C.c_ulong), ("ms", C.c_double)]


class spmvAmgOpts(C.Structure):
    """include/spmvHip.h `spmvAmgOpts` (a field 0: the built-in default; SPMV_AMG_NO_SWEEPS: no sweeps)."""
    _fields_ = [("seed", C.c_uint32), ("coarseRows", C.c_ulong), ("maxLevels", C.c_uint), ("omega", C.c_double),
                ("nu1", C.c_uint), ("nu2", C.c_uint), ("nuCoarse", C.c_uint)]


class spmvAmgInfo(C.Structure):
    """include/spmvHip.h `spmvAmgInfo`: the levels of a hierarchy."""
    _fields_ = [("levels", C.c_uint), ("rows", C.c_ulong * SPMV_AMG_MAX_LEVELS), ("nnz", C.c_ulong * SPMV_AMG_MAX_LEVELS),
                ("aggregates", C.c_ulong * SPMV_AMG_MAX_LEVELS), ("opComplexity", C.c_double), ("bytes", C.c_ulong),
                ("tempBytes", C.c_ulong), ("ms", C.c_double)]


class spmvAmgSmoothOpts(C.Structure):
    """include/spmvHip.h `spmvAmgSmoothOpts`: the damping of the smoothed prolongator (0: (4/3) / rho_l per level)."""
    _fields_ = [("omegaP", C.c_double)]


class spmvAmgStrengthOpts(C.Structure):
    """include/spmvHip.h `spmvAmgStrengthOpts`: the strength threshold per level (0: 0.08, scaled by 0.5 per level)."""
    _fields_ = [("theta", C.c_double), ("thetaScale", C.c_double)]


SPMV_AMG_SMOOTHER_JACOBI, SPMV_AMG_SMOOTHER_CHEBYSHEV, SPMV_AMG_MAX_DEGREE = 0, 1, 64


class spmvAmgSmootherOpts(C.Structure):
    """include/spmvHip.h `spmvAmgSmootherOpts`: the smoother of the cycle and its sweep counts (a field 0: the default)."""
    _fields_ = [("kind", _i), ("nu1", C.c_uint), ("nu2", C.c_uint), ("nuCoarse", C.c_uint), ("eigRatio", C.c_double),
                ("lambdaScale", C.c_double)]


class spmvAmgSmootherInfo(C.Structure):
    """include/spmvHip.h `spmvAmgSmootherInfo`: the smoother of one level; dCoef is the device address of nCoef (a, b) pairs."""
    _fields_ = [("kind", _i), ("nu1", C.c_uint), ("nu2", C.c_uint), ("nuCoarse", C.c_uint), ("rho", C.c_double),
                ("lambdaMax", C.c_double), ("lambdaMin", C.c_double), ("nCoef", C.c_uint), ("dCoef", C.POINTER(C.c_double))]


SPMV_AMG_SMOOTHER_GAUSS_SEIDEL = 2


class spmvAmgGsOpts(C.Structure):
    """include/spmvHip.h `spmvAmgGsOpts`: the multicolour Gauss-Seidel smoother of the cycle (a field 0: the default)."""
    _fields_ = [("order", _i), ("seed", C.c_uint32), ("omega", C.c_double), ("oneWay", _i), ("levels", C.c_uint),
                ("nu1", C.c_uint), ("nu2", C.c_uint), ("nuCoarse", C.c_uint)]


class spmvAmgGsInfo(C.Structure):
    """include/spmvHip.h `spmvAmgGsInfo`: the Gauss-Seidel state of one level; dPerm (M words) and dColourPtr (colours + 1
    words) are device addresses."""
    _fields_ = [("active", _i), ("colours", C.c_uint), ("maxColourRows", C.c_ulong), ("longRows", C.c_ulong), ("small", _i),
                ("omega", C.c_double), ("order", _i), ("seed", C.c_uint32), ("oneWay", _i), ("dPerm", C.POINTER(C.c_uint32)),
                ("dColourPtr", C.POINTER(C.c_uint32))]


class spmvAmgBlockInfo(C.Structure):
    """include/spmvHip.h `spmvAmgBlockInfo`: the width of a hierarchy's block workspace and its bytes (zeros: none)."""
    _fields_ = [("width", C.c_uint), ("bytes", C.c_ulong)]


class spmvAmgStorageInfo(C.Structure):
    """include/spmvHip.h `spmvAmgStorageInfo`: a hierarchy's storage, its levels and the bytes of its f32 forms (0 in F64)."""
    _fields_ = [("storage", _i), ("levels", C.c_uint), ("f32Bytes", C.c_ulong)]


class spmvAllocStats(C.Structure):
    """include/spmvHip.h `spmvAllocStats`: the ledger of the library's device allocations (for tests)."""
    _fields_ = [("live", C.c_ulong), ("liveBytes", C.c_ulong), ("peakBytes", C.c_ulong), ("calls", C.c_ulong),
                ("refused", C.c_ulong), ("badFrees", C.c_ulong)]


SPMV_COLOUR_NATURAL, SPMV_COLOUR_HASH = 0, 1
COLOUR_ORDERS = {"natural": SPMV_COLOUR_NATURAL, "hash": SPMV_COLOUR_HASH}
SPMV_RCM_START_MIN_DEGREE, SPMV_RCM_START_PERIPHERAL = 0, 1
RCM_STARTS = {"min_degree": SPMV_RCM_START_MIN_DEGREE, "peripheral": SPMV_RCM_START_PERIPHERAL}
SPMV_KRYLOV_CONVERGED, SPMV_KRYLOV_MAXITER, SPMV_KRYLOV_BREAKDOWN, SPMV_KRYLOV_NONFINITE = 0, 1, 2, 3
KRYLOV_STATUS = {0: "converged", 1: "maxiter", 2: "breakdown", 3: "nonfinite"}

IPC_HANDLE_BYTES = 64
MAX_PEERS = 15
for _name, (_args, _res) in _sigs.items():
    _f = getattr(lib, _name, None)
    if _f is None and os.environ.get("SPMV_LIB"):        # an older tuning build for an A/B may lack the newest entry points
        continue
    if _f is None:
        raise SpmvHipError(f"{LIB_PATH} does not export {_name}: rebuild it (`make lib`)")
    _f.argtypes, _f.restype = _args, _res

_hsigs = {
    "MMtoCSR": ([C.c_char_p], C.POINTER(spmat)), "MMtoELL": ([C.c_char_p], C.POINTER(spmat)),
    "freeSpmat": ([C.POINTER(spmat)], None),
    "ellTranspose": ([C.POINTER(spmat)], C.POINTER(spmat)),
    "csrToEll": ([C.POINTER(spmat)], C.POINTER(spmat)),
    "doubleVectorsDiff": ([_vp, _vp, C.c_ulong, C.POINTER(C.c_double)], _i),
    "statsAvgVar": ([_vp, C.c_uint, _vp], None),
    "fillRndVector": ([C.c_ulong, _vp], _i),
    "spmvModeFromString": ([C.c_char_p], _i),
    "writeDoubleVector": ([C.c_char_p, _vp, C.c_ulong], _i),
    "readDoubleVector": ([C.c_char_p, C.POINTER(C.c_ulong)], C.POINTER(C.c_double)),
    "spmvSynthPowerLawLengths": ([_u64, _u64, C.c_uint32, _u64, _vp, C.POINTER(C.c_double)], _i),
    "spmvSynthPrefix": ([_vp, _u64, _vp], _u64),
    "spmvSynthMakeX": ([_u64, _u64, _vp], None),
    "spmvSynthPerm": ([_u64, _u64, _u64], _u64),
    "spmvSynthWriteMtx": ([C.c_char_p, _i, C.c_ulong, C.c_ulong, C.c_ulong, _u64, C.POINTER(C.c_ulong), C.POINTER(C.c_ulong),
                           C.POINTER(C.c_ulong)], _i),
    "spmvSynthStructuredValue": ([_u64, C.c_ulong, C.c_ulong], C.c_double),
}
for _name, (_args, _res) in _hsigs.items():
    _f = getattr(hostlib, _name)
    _f.argtypes, _f.restype = _args, _res

SPMV_LAUNCHERS = {
    "hipSpMVRowsCSR": lib.hipSpMVRowsCSR,
    "hipSpMVWarpPerRowCSR": lib.hipSpMVWarpPerRowCSR,
    "hipSpMVRowsCSRf32": getattr(lib, "hipSpMVRowsCSRf32", None),           # (the products of the single-precision value form:
    "hipSpMVWarpPerRowCSRf32": getattr(lib, "hipSpMVWarpPerRowCSRf32", None),   # values_f32() first; None only in an older
                                                                            # tuning build loaded through SPMV_LIB).  The third f32 SpMV
    # entry point, spmvHipEnqueueRowsF32, takes (handle, x, y, stream) -- no CONFIG -- and so cannot stand in this table of
    # (handle, x, CONFIG, y) callables: it is bound in _sigs and called as lib.spmvHipEnqueueRowsF32.
    "hipSpMVTilesCSR": lib.hipSpMVTilesCSR,
    "hipSpMVStripesCSR": lib.hipSpMVStripesCSR,
    "hipSpMVAutoCSR": lib.hipSpMVAutoCSR,
    "hipSpMVRowsSELL": lib.hipSpMVRowsSELL,
    "hipSpMVRowsELL": lib.hipSpMVRowsELL,
    "hipSpMVRowsELLNNTransposed": lib.hipSpMVRowsELLNNTransposed,
    "hipSpMVWarpsPerRowELLNTrasposed": lib.hipSpMVWarpsPerRowELLNTrasposed,
}


def _check(rc, what):
    if rc != 0:
        raise SpmvHipError(f"{what} failed (EXIT_FAILURE) -- see stderr")


def _sweep_count(s):
    """a sweep count for the C boundary: a negative one cannot pass as a large unsigned"""
    s = int(s)
    if s < 0:
        raise ValueError(f"sweeps = {s} is negative")
    return s


def alloc_refuse(n=-1, from_then_on=False):
    """spmvHipAllocRefuse (for tests): the n-th device allocation from now (0-based) fails, with from_then_on every later
    one too; n = -1 disarms.  The ledger's calls and refused start again at 0 either way."""
    _check(lib.spmvHipAllocRefuse(int(n), 1 if from_then_on else 0), "spmvHipAllocRefuse")


def alloc_stats():
    """spmvHipAllocStats (for tests): the ledger of the library's device allocations as a spmvAllocStats"""
    st = spmvAllocStats()
    _check(lib.spmvHipAllocStats(C.byref(st)), "spmvHipAllocStats")
    return st


@contextlib.contextmanager
def alloc_refused(n, from_then_on=False):
    """`with alloc_refused(n): call` -- the call's n-th device allocation fails; disarmed on the way out, whatever happens"""
    alloc_refuse(n, from_then_on)
    try:
        yield
    finally:
        alloc_refuse(-1)


def _amg_sweeps(v):
    """a sweep count for spmvAmgOpts / spmvAmgSmootherOpts: None is the C side's 0 (its default, or what is kept), 0 asks for none"""
    return 0 if v is None else SPMV_AMG_NO_SWEEPS if int(v) == 0 else int(v)


def _ptr(a):
    """the address of a numpy array for a C call (None stays NULL); the caller keeps the array alive across the call"""
    return C.c_void_p(a.ctypes.data) if a is not None else None


_torch_module = None                                 # torch, once _torch() has found it


def _torch():
    """torch, imported at its first use (numpy arrays and raw pointers need none); None where it is not installed"""
    global _torch_module
    if _torch_module is None:
        try:
            import torch
            _torch_module = torch
        except ImportError:
            pass
    return _torch_module


def _device_vector(who, name, t, n=None, int32=False):
    """The one rule for a 1-D operand of a device call: a float64 (a permutation: int32) torch tensor on the device with
    dim() == 1 and unit stride -- any element offset, so a `[1:]` view passes and a `[::2]` view does not -- and of
    length n where n is given.  (With dim() == 1, is_contiguous() is that stride rule: it does not look at the offset,
    and a stride only counts where there is more than one element.)  Returns the length."""
    torch = _torch()
    if torch is None or not isinstance(t, torch.Tensor) or t.dtype != (torch.int32 if int32 else torch.float64) or not t.is_cuda \
            or t.dim() != 1 or not t.is_contiguous():
        kind = "a DeviceBuffer of uint32 or a 1-D int32" if int32 else "a 1-D float64"
        raise SpmvHipError(f"{who}: {name} must be {kind} torch tensor on the device with unit stride")
    length = t.numel()
    if n is not None and length != n:
        raise SpmvHipError(f"{who}: {name} must have length {n}, not {length}")
    return length


class _Operands:
    """The operands of one call into the library, for every entry point that takes numpy arrays or device tensors.

    The first operand decides the kind of the call: a numpy array makes it a host call (inputs are uploaded into one
    temporary DeviceBuffer that also holds the result, which is downloaded as numpy), anything else a device call (torch tensors are read and written
    where they live, the result is a tensor).  Every other operand must be of the same kind.  Use:

        with _Operands("who", first) as ops:
            ops.vector(...)                  # the inputs in the order of the C arguments: each is CHECKED, nothing more
            ops.result(...)                  # the result ends the declarations: checked, then a host call makes its buffer
            _check(lib.X(..., *ops.args), "X")       # ops.args: the device addresses, in the order of declaration
            return ops.value()               # `out` or the new tensor; a host call downloads its numpy result

    so a refused call has made no device call at all, and the temporaries are freed on success and on every failure.
    With no operand (colour, permute, aggregate) it is only the scope that frees what temp() made."""
    __slots__ = ("who", "host", "first", "args", "tmp", "res")       # res: the result tensor, or a host call's result shape

    def __init__(self, who, first=None, host_calls=True):
        self.who, self.first, self.host, self.args, self.tmp, self.res = who, first, isinstance(first, np.ndarray), [], [], None
        if self.host and not host_calls:
            raise SpmvHipError(f"{who}: the operands must be torch tensors on the device")

    def __enter__(self):
        return self

    def __exit__(self, kind, error, trace):
        for b in self.tmp:
            b.free()

    def temp(self, nbytes, host=None):
        """a DeviceBuffer that lives until the call is over, filled from the host array when one is given"""
        buf = DeviceBuffer(nbytes)
        self.tmp.append(buf)
        return buf if host is None else buf.up(host)

    def keep(self):
        """the buffers made so far are the call's result: they outlive it"""
        self.tmp = []

    def _host(self, name, a, shape):
        if not isinstance(a, np.ndarray) or a.shape != shape:
            raise SpmvHipError(f"{self.who}: {name} must be a numpy array of shape {shape}, as this is a host call")
        return np.ascontiguousarray(a, dtype=np.float64)

    def vector(self, name, v, n=None, least=0):
        """an input vector of length n (any length: None); returns the length"""
        if not self.host:
            n = _device_vector(self.who, name, v, n)
            self.args.append(v.data_ptr())
            return n
        h = self._host(name, v, (n,))
        self.args.append((h, least))
        return h.size

    def triplets(self, name, a, n=None, index=False):
        """an operand of the triplet calls, which have no result vector to share a buffer with: the values (float64), or with
        index=True a row / column array.  Host call: a 1-D numpy array, an index array of any integer dtype with every
        element -1 (the skip marker) or in [0, 2^32 - 1]; it is checked, then uploaded as float64 / uint32 into a temp() of
        its own.  Device call: a float64 / int32 tensor under the 1-D rule, used where it lives (-1 is the skip marker's
        bits).  Appends the device address; returns the length."""
        if not self.host:
            n = _device_vector(self.who, name, a, n, int32=index)
            self.args.append(a.data_ptr())
            return n
        if not isinstance(a, np.ndarray) or a.ndim != 1 or (n is not None and a.size != n):
            raise SpmvHipError(f"{self.who}: {name} must be a 1-D numpy array" + (f" of length {n}" if n is not None else "")
                               + ", as this is a host call")
        if index:
            if not np.issubdtype(a.dtype, np.integer):
                raise SpmvHipError(f"{self.who}: {name} must hold integers, not {a.dtype}")
            skip = a == -1 if np.issubdtype(a.dtype, np.signedinteger) else np.zeros(a.shape, bool)
            if a.size and not np.all(skip | ((a >= 0) & (a <= SPMV_COO_SKIP))):
                raise SpmvHipError(f"{self.who}: {name} holds a value that is neither -1 nor in [0, 2^32 - 1]")
            h = np.where(skip, SPMV_COO_SKIP, a).astype(np.uint32)
        else:
            h = np.ascontiguousarray(a, dtype=np.float64)
        self.args.append(self.temp(h.nbytes, h if h.size else None).ptr.value)
        return h.size

    def dense(self, name, X, rows):
        """matmul's X, (rows, k) with k >= 1: (k, layout, leading dimension)"""
        if self.host:
            ok = X.ndim == 2
        else:
            torch = _torch()
            if torch is None or not isinstance(X, torch.Tensor):
                raise SpmvHipError(f"{self.who}: {name} must be a numpy array or a torch tensor")
            ok = X.dim() == 2
        if not ok or X.shape[0] != rows or X.shape[1] < 1:
            raise SpmvHipError(f"{self.who}: {name} must be ({rows}, k) with k >= 1, not {tuple(X.shape)}")
        k = X.shape[1]
        if self.host:
            h = np.ascontiguousarray(X, dtype=np.float64)
            self.args.append((h, 0))
            return k, SPMV_DENSE_ROW_MAJOR, k
        layout, ld = _dense_layout(X, name, self.who)
        self.args.append(X.data_ptr())
        return k, layout, ld

    def columns(self, name, V):
        """multi_dot's V, (n, k) with contiguous columns: (n, k, leading dimension)"""
        if self.host:
            if V.ndim != 2 or V.shape[1] < 1:
                raise SpmvHipError(f"{self.who}: {name} must be (n, k) with k >= 1, not {V.shape}")
            self.args.append((np.asfortranarray(V, dtype=np.float64).ravel(order="F"), 8))
            return V.shape[0], V.shape[1], V.shape[0]
        torch = _torch()
        if torch is None or not isinstance(V, torch.Tensor) or V.dtype != torch.float64 or not V.is_cuda or V.dim() != 2:
            raise SpmvHipError(f"{self.who}: {name} must be a 2-D float64 torch tensor on the device")
        n, k = V.shape
        if (n > 1 and V.stride(0) != 1) or (k > 1 and V.stride(1) < n):
            raise SpmvHipError(f"{self.who}: {name} needs contiguous columns (strides {V.stride()})")
        self.args.append(V.data_ptr())
        return n, k, V.stride(1) if k > 1 else max(n, 1)

    def result(self, name, out, shape, init=None, least=0):
        """The result; it ends the declarations.  Host call: `out` is refused; every operand is checked by now, so the
        call's buffer is made here and the inputs are uploaded.  Device call: `out` under the rule of its rank, else a new tensor.
        init=(name, x0): the result starts as a copy of that operand, zeros when x0 is None, and x0 itself is never
        written; init=None: it starts uninitialised.  Returns (layout, leading dimension) of a 2-D result."""
        if self.host:
            if out is not None:
                raise SpmvHipError(f"{self.who}: `{name}` is for device calls; a host call returns a new numpy array")
            start = None
            if init is not None:
                start = np.zeros(shape) if init[1] is None else self._host(init[0], init[1], shape)
            arrays, offsets, total = [h for h, _ in self.args] + [start], [], 0
            for n in [max(h.nbytes, atleast) for h, atleast in self.args] + [max(8 * math.prod(shape), least)]:
                offsets.append(total)                    # one allocation for the call, every operand on a 256-byte boundary
                total += (max(n, 1) + 255) // 256 * 256
            base = self.temp(total).ptr.value
            self.args = [base + o for o in offsets]
            for h, address in zip(arrays, self.args):
                if h is not None and h.nbytes:
                    _check(lib.spmvHipMemcpyUp(address, _ptr(h), h.nbytes), "spmvHipMemcpyUp")
            self.res = shape
            return (SPMV_DENSE_ROW_MAJOR, shape[1]) if len(shape) == 2 else None
        if out is not None:
            if len(shape) == 1:
                _device_vector(self.who, name, out, shape[0])
            elif not isinstance(out, _torch().Tensor) or out.dim() != 2 or tuple(out.shape) != shape:
                raise SpmvHipError(f"{self.who}: {name} must be a torch tensor of shape {shape}")
        elif init is None:                               # (the first operand is a float64 tensor on the device by now)
            out = self.first.new_empty(shape)
        elif init[1] is None:
            out = self.first.new_zeros(shape)
        else:
            if len(shape) == 1:
                _device_vector(self.who, init[0], init[1], shape[0])
            elif not isinstance(init[1], _torch().Tensor) or tuple(init[1].shape) != shape:
                raise SpmvHipError(f"{self.who}: {init[0]} must be a torch tensor of shape {shape}")
            else:
                _dense_layout(init[1], init[0], self.who)
            out = init[1].clone()
        self.res = out
        self.args.append(out.data_ptr())
        return _dense_layout(out, name, self.who) if len(shape) == 2 else None

    def value(self):
        """after the C call: the result tensor, or the host call's result downloaded (nothing is copied for an empty one)"""
        assert self.res is not None, "result() was not declared"
        if not self.host:
            return self.res
        out = np.empty(self.res)
        if out.size:
            _check(lib.spmvHipMemcpyDown(_ptr(out), self.args[-1], out.nbytes), "spmvHipMemcpyDown")
        return out


# ----------------------------------------------------------------- lifecycle
def spmvHipInit(dev=0):
    _check(lib.spmvHipInit(int(dev), C.sizeof(spmat), C.sizeof(CONFIG)), "spmvHipInit")


def spmvHipFinalize():
    lib.spmvHipFinalize()


# ----------------------------------------------------------------- host matrices
class HostCSR:
    """A host `spmat` in CSR form over numpy arrays (64-bit indices like the
    reference's loader output).  Keeps the arrays alive."""

    def __init__(self, M, N, IRP, JA, AS, with_row_lens=True):
        self.IRP = np.ascontiguousarray(IRP, dtype=np.uint64)
        self.JA = np.ascontiguousarray(JA, dtype=np.uint64)
        self.AS = np.ascontiguousarray(AS, dtype=np.float64)
        assert self.IRP.shape == (M + 1,) and self.JA.shape == self.AS.shape
        self.RL = np.diff(self.IRP).astype(np.uint64) if with_row_lens else None
        s = spmat()
        s.M, s.N, s.NZ = M, N, int(self.JA.size)
        s.IRP = self.IRP.ctypes.data_as(C.POINTER(C.c_ulong))
        s.JA = self.JA.ctypes.data_as(C.POINTER(C.c_ulong))
        s.AS = self.AS.ctypes.data_as(C.POINTER(C.c_double))
        if self.RL is not None:
            s.RL = self.RL.ctypes.data_as(C.POINTER(C.c_ulong))
        self.struct = s

    @property
    def M(self):
        return self.struct.M

    @property
    def N(self):
        return self.struct.N

    @property
    def NZ(self):
        return self.struct.NZ

    def to_ell(self, with_row_lens=True):
        """Row-major ELL with {JA=0, AS=0} padding (parser.c:246-253 semantics)."""
        M = self.M
        lens = np.diff(self.IRP).astype(np.int64)
        K = int(lens.max()) if M else 0
        JA = np.zeros((M, K), dtype=np.uint64)
        AS = np.zeros((M, K), dtype=np.float64)
        if self.NZ:
            rows = np.repeat(np.arange(M), lens)
            pos = np.arange(self.NZ) - np.repeat(self.IRP[:-1].astype(np.int64), lens)
            JA[rows, pos] = self.JA
            AS[rows, pos] = self.AS
        return HostELL(M, self.N, self.NZ, K, JA, AS, lens.astype(np.uint64) if with_row_lens else None)


class HostELL:
    """A host `spmat` in ELL form.  `transposed` follows the reference's
    ellTranspose field convention (sparseUtils.c:168-171)."""

    def __init__(self, M, N, NZ, K, JA, AS, RL=None, transposed=False):
        self.JA = np.ascontiguousarray(JA, dtype=np.uint64)
        self.AS = np.ascontiguousarray(AS, dtype=np.float64)
        self.RL = None if RL is None else np.ascontiguousarray(RL, dtype=np.uint64)
        self.rows, self.slots, self.transposed = M, K, transposed
        s = spmat()
        s.NZ = NZ
        if transposed:
            s.M, s.N, s.MAX_ROW_NZ = K, M, M
            s.dev = SPMAT_TAG_ELL_TRANSPOSED
            s.pitchJA = N                       # column count for the upload's range check (see ellTranspose)
        else:
            s.M, s.N, s.MAX_ROW_NZ = M, N, K
        s.JA = self.JA.ctypes.data_as(C.POINTER(C.c_ulong))
        s.AS = self.AS.ctypes.data_as(C.POINTER(C.c_double))
        if self.RL is not None:
            s.RL = self.RL.ctypes.data_as(C.POINTER(C.c_ulong))
        self.struct = s
        self._N = N

    def transpose(self):
        """ellTranspose (sparseUtils.c:145-185) on numpy arrays."""
        assert not self.transposed
        return HostELL(self.rows, self._N, self.struct.NZ, self.slots,
                       self.JA.reshape(self.rows, self.slots).T.copy(),
                       self.AS.reshape(self.rows, self.slots).T.copy(), self.RL, transposed=True)


# ----------------------------------------------------------------- device objects
class _DeviceMemory:
    """what DeviceVector and DeviceBuffer share: `ptr` goes back to the allocator once, by free() or with the object"""
    _release = None

    def free(self):
        if self.ptr:
            self._release(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceVector(_DeviceMemory):
    _release = staticmethod(lib.spmvHipVecFree)

    def __init__(self, n):
        self.n = int(n)
        p = C.c_void_p()
        _check(lib.spmvHipVecAlloc(C.byref(p), self.n), "spmvHipVecAlloc")
        self.ptr = p

    def up(self, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        assert host.size == self.n
        _check(lib.spmvHipVecUp(self.ptr, _ptr(host), self.n), "spmvHipVecUp")
        return self

    def down(self):
        out = np.empty(self.n, dtype=np.float64)
        _check(lib.spmvHipVecDown(_ptr(out), self.ptr, self.n), "spmvHipVecDown")
        return out

    def poison(self):
        _check(lib.spmvHipVecFill(self.ptr, self.n, POISON_NAN), "spmvHipVecFill")


class DeviceBuffer(_DeviceMemory):
    """Raw device bytes (for device-format matrices built on the GPU)."""
    _release = staticmethod(lib.spmvHipFree)

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(lib.spmvHipMalloc(C.byref(p), max(self.nbytes, 1)), "spmvHipMalloc")
        self.ptr = p

    def up(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        _check(lib.spmvHipMemcpyUp(self.ptr, _ptr(host), self.nbytes), "spmvHipMemcpyUp")
        return self

    def down(self, dtype):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(lib.spmvHipMemcpyDown(_ptr(out), self.ptr, self.nbytes), "spmvHipMemcpyDown")
        return out


class DeviceMatrix:
    """A device handle (`spmat` whose `dev` is set) plus what keeps it alive."""

    def __init__(self):
        self.handle = spmat()
        self.keep = []
        self.rows = 0

    def update_values(self, AS, on_device=False):
        """spmvHipUpdateValues: new values for the same pattern, in the handle's value layout (CSR: NZ values in CSR order;
        uploaded ELL: the host ELL value array of the upload).  AS: a numpy array (host), a float64 torch tensor (read
        where it lives) or a raw device pointer (int / c_void_p, with on_device=True)."""
        torch = _torch()                                 # (None without torch: numpy arrays and raw pointers need none)
        keep = None
        if torch is not None and isinstance(AS, torch.Tensor):
            if AS.dtype != torch.float64 or not AS.is_contiguous():
                raise SpmvHipError("update_values: the tensor must be contiguous float64")
            ptr, on_device = C.c_void_p(AS.data_ptr()), AS.is_cuda
        elif isinstance(AS, np.ndarray):
            keep = np.ascontiguousarray(AS, dtype=np.float64)
            ptr, on_device = _ptr(keep), False
        else:
            ptr = AS if isinstance(AS, C.c_void_p) else C.c_void_p(int(AS))
        _check(lib.spmvHipUpdateValues(C.byref(self.handle), ptr, 1 if on_device else 0), "spmvHipUpdateValues")

    def values_changed(self):
        """spmvHipValuesChanged: the handle's own value array (an adopted dAS) was rewritten on the device."""
        _check(lib.spmvHipValuesChanged(C.byref(self.handle)), "spmvHipValuesChanged")

    def values_f32(self, on=True):
        """spmvHipValuesF32: build (or, on=False, release) the single-precision form of this CSR matrix's values, 4 B per
        entry beside the doubles: AS32[p] = (float)AS[p], round to nearest even.  The f32 launchers (`spmv` with
        "hipSpMVRowsCSRf32" / "hipSpMVWarpPerRowCSRf32", `matmul(values="f32")`) stream it and compute in double; it follows
        every later change of the values.  Idempotent."""
        _check(lib.spmvHipValuesF32(C.byref(self.handle), 1 if on else 0), "spmvHipValuesF32")

    def values_f32_info(self) -> "spmvF32Info":
        """spmvHipValuesF32Info: built, unit, bytes, refreshes, and what the build or the last refresh rounded: inexact,
        overflowed, flushed, firstOverflow."""
        info = spmvF32Info()
        _check(lib.spmvHipValuesF32Info(C.byref(self.handle), C.byref(info)), "spmvHipValuesF32Info")
        return info

    def update_info(self) -> "spmvUpdateInfo":
        """spmvHipLastUpdateInfo: what the last update_values / values_changed did."""
        info = spmvUpdateInfo()
        _check(lib.spmvHipLastUpdateInfo(C.byref(self.handle), C.byref(info)), "spmvHipLastUpdateInfo")
        return info

    def transpose(self) -> "DeviceMatrix":
        """spmvHipCsrTranspose: A^T built on the device as a new DeviceMatrix that owns its handle.  Row j holds the entries
        of column j in CSR position order, so hipSpMVRowsCSR on it gives the bits of the serial scatter loop y[JA[p]] +=
        AS[p] * x[i].  Refresh its values after this matrix's change with `refresh_from(self)`."""
        t = DeviceMatrix()
        _check(lib.spmvHipCsrTranspose(C.byref(self.handle), C.byref(t.handle)), "spmvHipCsrTranspose")
        t.rows = int(t.handle.M)
        return t

    def refresh_from(self, source: "DeviceMatrix"):
        """spmvHipTransposeRefresh: this transpose takes `source`'s current device values (source must be the matrix it
        was transposed from), then refreshes its formats as values_changed() does."""
        _check(lib.spmvHipTransposeRefresh(C.byref(self.handle), C.byref(source.handle)), "spmvHipTransposeRefresh")

    def colour(self, order="natural", seed=0, want_colours=False, as_torch=False) -> "Colouring":
        """spmvHipColourCSR: a multi-colour ordering of this square matrix, a function of its pattern and (order, seed) alone
        (include/spmvHip.h states the loop).  Returns a Colouring: `perm` (rows by (colour, id), perm[new] = old: the
        argument of permute() and permute_vector()), `colours` (per row, when want_colours), `info` (spmvColourInfo) and
        free().  perm / colours are DeviceBuffers of uint32, or int32 device torch tensors with as_torch=True."""
        if order not in COLOUR_ORDERS:
            raise SpmvHipError(f"colour: order must be one of {sorted(COLOUR_ORDERS)}, not {order!r}")
        M = int(self.handle.M)
        opts, info = spmvColourOpts(COLOUR_ORDERS[order], int(seed) & 0xFFFFFFFF), spmvColourInfo()
        with _Operands("colour") as ops:                 # no operand: the scope that frees the buffers if the call fails
            if as_torch:
                torch = _torch()
                perm = torch.empty(M, dtype=torch.int32, device="cuda")
                colours = torch.empty(M, dtype=torch.int32, device="cuda") if want_colours else None
            else:
                perm = ops.temp(4 * M)
                colours = ops.temp(4 * M) if want_colours else None
            _check(lib.spmvHipColourCSR(C.byref(self.handle), C.byref(opts), _dev_ptr(colours), _dev_ptr(perm), C.byref(info)),
                   "spmvHipColourCSR")
            ops.keep()                                   # the Colouring owns the buffers from here
        return Colouring(perm, colours, info)

    def rcm(self, start="peripheral", max_passes=0, forward=False, as_torch=False) -> "Ordering":
        """spmvHipRcmCSR: the reverse Cuthill-McKee ordering of this square matrix, a function of its pattern and the options
        alone (include/spmvHip.h states the loop).  start: "peripheral" or "min_degree"; max_passes: BFS runs of the start
        search per component (0: 8); forward: the unreversed order.  Returns an Ordering: `perm` (perm[new] = old: the
        argument of permute() and permute_vector()), `info` (spmvRcmInfo) and free().  perm is a DeviceBuffer of uint32, or
        an int32 device torch tensor with as_torch=True."""
        if start not in RCM_STARTS:
            raise SpmvHipError(f"rcm: start must be one of {sorted(RCM_STARTS)}, not {start!r}")
        M = int(self.handle.M)
        opts, info = spmvRcmOpts(RCM_STARTS[start], int(max_passes), 1 if forward else 0), spmvRcmInfo()
        with _Operands("rcm") as ops:                    # no operand: the scope that frees the buffer if the call fails
            perm = _torch().empty(M, dtype=_torch().int32, device="cuda") if as_torch else ops.temp(4 * M)
            _check(lib.spmvHipRcmCSR(C.byref(self.handle), C.byref(opts), _dev_ptr(perm), C.byref(info)), "spmvHipRcmCSR")
            ops.keep()                                   # the Ordering owns the buffer from here
        return Ordering(perm, info)

    def permute(self, perm) -> "DeviceMatrix":
        """spmvHipCsrPermute: B = P A P^T as a new DeviceMatrix that owns its handle; row r of B is row perm[r] of this
        matrix, columns renumbered alike and sorted ascending (stable for repeats).  perm: a Colouring, an Ordering, a
        DeviceBuffer of M uint32, an int32 device torch tensor, or a numpy array (uploaded for the call)."""
        M = int(self.handle.M)
        perm = perm.perm if isinstance(perm, (Colouring, Ordering)) else perm
        b = DeviceMatrix()
        with _Operands("permute") as ops:                # no operand: the scope that frees an uploaded perm
            if isinstance(perm, np.ndarray):
                if perm.shape != (M,):
                    raise SpmvHipError(f"permute: perm must have shape ({M},), not {perm.shape}")
                perm = ops.temp(4 * M, np.ascontiguousarray(perm, dtype=np.uint32))
            elif _perm_len(perm, "permute") != M:
                raise SpmvHipError(f"permute: perm must hold {M} entries")
            _check(lib.spmvHipCsrPermute(C.byref(self.handle), _dev_ptr(perm), C.byref(b.handle)), "spmvHipCsrPermute")
        b.rows = int(b.handle.M)
        return b

    def permute_refresh(self, source: "DeviceMatrix"):
        """spmvHipPermuteRefresh: this permuted matrix takes `source`'s current device values (source must be the matrix it
        was permuted from), then refreshes its formats as values_changed() does."""
        _check(lib.spmvHipPermuteRefresh(C.byref(self.handle), C.byref(source.handle)), "spmvHipPermuteRefresh")

    def multiply(self, other: "DeviceMatrix", waveMaxProducts=0, groupMaxProducts=0, sortBudgetBytes=0) -> "DeviceMatrix":
        """spmvHipSpGEMM: C = self * other as a new DeviceMatrix that owns its handle, bit for bit the serial loop of
        include/spmvHip.h (terms in stored (p, q) order, rows of C ascending, structural zeros kept).  The options only
        lower the class limits (0: the defaults).  `other` may be this matrix.  spgemm_info() tells what the call did."""
        c = DeviceMatrix()
        opts, info = spmvSpgemmOpts(int(waveMaxProducts), int(groupMaxProducts), int(sortBudgetBytes)), spmvSpgemmInfo()
        _check(lib.spmvHipSpGEMM(C.byref(self.handle), C.byref(other.handle), C.byref(opts), C.byref(c.handle), C.byref(info)),
               "spmvHipSpGEMM")
        c.rows = int(c.handle.M)
        c._spgemm = info
        return c

    def multiply_refresh(self, a: "DeviceMatrix", b: "DeviceMatrix"):
        """spmvHipSpGEMMRefresh: this product takes its values again from the current values of `a` and `b` (the pair it
        was built from, in that order), pattern and addresses kept, then refreshes its formats as values_changed() does."""
        info = spmvSpgemmInfo()
        _check(lib.spmvHipSpGEMMRefresh(C.byref(self.handle), C.byref(a.handle), C.byref(b.handle), C.byref(info)),
               "spmvHipSpGEMMRefresh")
        self._spgemm = info

    def spgemm_info(self) -> "spmvSpgemmInfo":
        """the spmvSpgemmInfo of the multiply() that made this matrix, or of its last multiply_refresh()"""
        info = getattr(self, "_spgemm", None)
        if info is None:
            raise SpmvHipError("spgemm_info: this matrix was not made by multiply()")
        return info

    def add(self, other: "DeviceMatrix", alpha=1.0, beta=1.0, laneMaxTerms=0, waveMaxTerms=0, sortBudgetBytes=0,
            allSorted=False) -> "DeviceMatrix":
        """spmvHipCsrAdd: C = alpha * self + beta * other as a new DeviceMatrix that owns its handle, bit for bit the serial
        loop of include/spmvHip.h (self's terms of a row in stored order, then other's; rows of C ascending; structural zeros
        kept).  The options only lower the class limits (0: the defaults); allSorted sends every row down the general path.
        `other` may be this matrix.  add_info() tells what the call did."""
        c = DeviceMatrix()
        opts = spmvAddOpts(int(laneMaxTerms), int(waveMaxTerms), int(sortBudgetBytes), int(bool(allSorted)))
        info = spmvAddInfo()
        _check(lib.spmvHipCsrAdd(float(alpha), C.byref(self.handle), float(beta), C.byref(other.handle), C.byref(opts),
                                 C.byref(c.handle), C.byref(info)), "spmvHipCsrAdd")
        c.rows = int(c.handle.M)
        c._add = info
        return c

    def add_refresh(self, a: "DeviceMatrix", b: "DeviceMatrix", alpha=1.0, beta=1.0):
        """spmvHipCsrAddRefresh: this sum takes its values again as alpha * a + beta * b from the current values of `a` and
        `b` (the pair it was built from, in that order; alpha and beta may be new), pattern and addresses kept, then
        refreshes its formats as values_changed() does."""
        info = spmvAddInfo()
        _check(lib.spmvHipCsrAddRefresh(C.byref(self.handle), float(alpha), C.byref(a.handle), float(beta), C.byref(b.handle),
                                        C.byref(info)), "spmvHipCsrAddRefresh")
        self._add = info

    def add_info(self) -> "spmvAddInfo":
        """the spmvAddInfo of the add() that made this matrix, or of its last add_refresh()"""
        info = getattr(self, "_add", None)
        if info is None:
            raise SpmvHipError("add_info: this matrix was not made by add()")
        return info

    def filter(self, mode, lo=None, hi=None, theta=0.0, lump=False) -> "DeviceMatrix":
        """spmvHipCsrFilter: the entries of this matrix that a predicate keeps, in stored order, values copied as bits, as a
        new DeviceMatrix that owns its handle (include/spmvHip.h states the loop).  mode: "band" (lo <= j - i <= hi; None:
        the open end), "abs" (|a| > theta) or "strength" (j == i, or a * a > theta^2 |d_i d_j|), or a SPMV_FILTER_* value.
        lump: the dropped entries of a row are added, in stored order, to its diagonal entry.  filter_info() tells what the
        call did."""
        if isinstance(mode, str) and mode not in FILTER_MODES:
            raise SpmvHipError(f"filter: mode must be one of {sorted(FILTER_MODES)}, not {mode!r}")
        opts = spmvFilterOpts(FILTER_MODES[mode] if isinstance(mode, str) else int(mode), INT64_MIN if lo is None else int(lo),
                              INT64_MAX if hi is None else int(hi), float(theta), int(bool(lump)))
        c, info = DeviceMatrix(), spmvFilterInfo()
        _check(lib.spmvHipCsrFilter(C.byref(self.handle), C.byref(opts), C.byref(c.handle), C.byref(info)), "spmvHipCsrFilter")
        c.rows = int(c.handle.M)
        c._filter = info
        return c

    def filter_refresh(self, source: "DeviceMatrix"):
        """spmvHipCsrFilterRefresh: this filtered matrix takes `source`'s current values at the places kept at the build
        (nothing is judged again; with lump the diagonal is summed again over the build's dropped places), pattern and
        addresses kept, then refreshes its formats as values_changed() does."""
        info = spmvFilterInfo()
        _check(lib.spmvHipCsrFilterRefresh(C.byref(self.handle), C.byref(source.handle), C.byref(info)), "spmvHipCsrFilterRefresh")
        self._filter = info

    def filter_info(self) -> "spmvFilterInfo":
        """the spmvFilterInfo of the filter() that made this matrix, or of its last filter_refresh()"""
        info = getattr(self, "_filter", None)
        if info is None:
            raise SpmvHipError("filter_info: this matrix was not made by filter()")
        return info

    def assemble_refresh(self, vals):
        """spmvHipCooAssembleRefresh: this matrix, made by assemble_coo() with keep_map=True, takes new values for the SAME
        triplet list (same length, same order): the duplicates are added again in input order over the build's runs,
        pattern and addresses kept, then the formats are refreshed as values_changed() does.  vals: a numpy array
        (uploaded for the call) or a float64 device torch tensor (read where it lives)."""
        info = spmvCooInfo()
        with _Operands("assemble_refresh", vals) as ops:
            n = ops.triplets("vals", vals)
            _check(lib.spmvHipCooAssembleRefresh(C.byref(self.handle), n, *ops.args, C.byref(info)), "spmvHipCooAssembleRefresh")
        self._coo = info

    def assemble_info(self) -> "spmvCooInfo":
        """the spmvCooInfo of the assemble_coo() that made this matrix, or of its last assemble_refresh()"""
        info = getattr(self, "_coo", None)
        if info is None:
            raise SpmvHipError("assemble_info: this matrix was not made by assemble_coo()")
        return info

    def to_coo(self, as_torch=False):
        """spmvHipCsrToCoo: (rows, cols, vals) of the NZ stored entries of this CSR matrix in stored order: numpy arrays
        (uint32, uint32, float64), or with as_torch=True device torch tensors (int32, int32, float64) written in place."""
        NZ = int(self.handle.NZ)
        with _Operands("to_coo") as ops:                 # no operand: the scope that frees the download buffers
            if as_torch:
                torch = _torch()
                out = [torch.empty(NZ, dtype=t, device="cuda") for t in (torch.int32, torch.int32, torch.float64)]
            else:
                out = [ops.temp(4 * NZ), ops.temp(4 * NZ), ops.temp(8 * NZ)]
            _check(lib.spmvHipCsrToCoo(C.byref(self.handle), *[_dev_ptr(b) for b in out]), "spmvHipCsrToCoo")
            if as_torch:
                return tuple(out)
            return tuple(b.down(t) if NZ else np.zeros(0, t) for b, t in zip(out, (np.uint32, np.uint32, np.float64)))

    def tril(self, k=0) -> "DeviceMatrix":
        """the entries on and below the k-th diagonal (j - i <= k), as filter("band")"""
        return self.filter("band", hi=k)

    def triu(self, k=0) -> "DeviceMatrix":
        """the entries on and above the k-th diagonal (j - i >= k), as filter("band")"""
        return self.filter("band", lo=k)

    def diagonal_matrix(self) -> "DeviceMatrix":
        """the stored diagonal entries as a matrix of their own, as filter("band", 0, 0)"""
        return self.filter("band", lo=0, hi=0)

    def aggregate(self, seed=0):
        """spmvHipAggregateCSR: the aggregate id of every vertex of this square matrix, a function of its pattern and the
        seed alone (include/spmvHip.h states the loop).  Returns (ids, info): a numpy uint32 array and a spmvAggInfo."""
        M = int(self.handle.M)
        opts, info = spmvAggOpts(int(seed) & 0xFFFFFFFF), spmvAggInfo()
        with _Operands("aggregate") as ops:              # no operand: the scope that frees the id buffer
            buf = ops.temp(4 * M)
            _check(lib.spmvHipAggregateCSR(C.byref(self.handle), C.byref(opts), buf.ptr, C.byref(info)), "spmvHipAggregateCSR")
            return (buf.down(np.uint32) if M else np.zeros(0, np.uint32)), info

    def amg(self, seed=0, coarseRows=None, maxLevels=None, omega=None, nu1=None, nu2=None, nuCoarse=None, smoothed=False,
            omegaP=None, theta=None, thetaScale=None) -> "AmgHierarchy":
        """spmvHipAmgSetup: an aggregation multigrid hierarchy of this square matrix (include/spmvHip.h states the loops).
        None: the built-in default (512, 16, 2/3, 1, 1, 8); nu1 / nu2 / nuCoarse = 0 asks for no sweeps.  The result is
        accepted as `precond=` by cg / bicgstab / gmres of this matrix.  smoothed: spmvHipAmgSetupSmoothed, the
        prolongator T - omegaP D^-1 A T (omegaP None: (4/3) / rho_l per level).  theta or thetaScale given (with
        smoothed=True): spmvHipAmgSetupStrength, which aggregates and smooths on the strength-filtered matrix with the
        threshold theta * thetaScale^l on level l (None: 0.08, 0.5).  Stored in single precision: `A.amg(...).set_storage("f32")`."""
        opts = spmvAmgOpts(int(seed) & 0xFFFFFFFF, int(coarseRows or 0), int(maxLevels or 0), float(omega or 0.0), _amg_sweeps(nu1),
                           _amg_sweeps(nu2), _amg_sweeps(nuCoarse))
        h = AmgHierarchy(self)
        strength = theta is not None or thetaScale is not None
        if strength and not smoothed:
            raise SpmvHipError("amg: theta and thetaScale are the strength filter of the smoothed hierarchy (smoothed=True)")
        if strength:
            smooth, so = spmvAmgSmoothOpts(float(omegaP or 0.0)), spmvAmgStrengthOpts(float(theta or 0.0), float(thetaScale or 0.0))
            _check(lib.spmvHipAmgSetupStrength(C.byref(self.handle), C.byref(opts), C.byref(smooth), C.byref(so), C.byref(h.handle),
                                               C.byref(h.info)), "spmvHipAmgSetupStrength")
        elif smoothed:
            smooth = spmvAmgSmoothOpts(float(omegaP or 0.0))
            _check(lib.spmvHipAmgSetupSmoothed(C.byref(self.handle), C.byref(opts), C.byref(smooth), C.byref(h.handle), C.byref(h.info)),
                   "spmvHipAmgSetupSmoothed")
        else:
            if omegaP is not None:
                raise SpmvHipError("amg: omegaP is the damping of the smoothed prolongator (smoothed=True)")
            _check(lib.spmvHipAmgSetup(C.byref(self.handle), C.byref(opts), C.byref(h.handle), C.byref(h.info)), "spmvHipAmgSetup")
        h.rows = int(h.handle.M)
        return h

    def matmul(self, X, out=None, values="f64"):
        """hipSpMMRowsCSR: Y = A X, column c of Y bit-identical to sgemvSerial on column c of X; values="f32": hipSpMMRowsCSRf32,
        the same from the single-precision form of the values (`values_f32()` first), arithmetic in double.  X is (N, k) float64:
        a device torch tensor with unit stride in one dimension (a contiguous tensor is row-major, a `.t()` view of a
        contiguous (k, N) tensor column-major; the leading dimension is the other stride) -> a torch tensor, `out` if
        given (same rules); or a numpy array -> uploaded, multiplied, returned as numpy.  Runs on the library stream."""
        M, N = int(self.handle.M), int(self.handle.N)
        with _Operands("matmul", X) as ops:
            k, xl, ldx = ops.dense("X", X, N)
            yl, ldy = ops.result("out", out, (M, k))
            dx, dy = ops.args
            name = "hipSpMMRowsCSRf32" if _storage(values, "matmul") else "hipSpMMRowsCSR"
            _check(getattr(lib, name)(C.byref(self.handle), k, dx, ldx, xl, dy, ldy, yl), name)
            return ops.value()

    def triangular_analyse(self, lower=True):
        """spmvHipTriAnalyse: build the level-set schedule of the lower (or upper) triangle now (the first solve does it
        otherwise); a no-op when it exists."""
        _check(lib.spmvHipTriAnalyse(C.byref(self.handle), SPMV_TRI_LOWER if lower else SPMV_TRI_UPPER), "spmvHipTriAnalyse")

    def triangular_info(self, lower=True) -> "spmvTriInfo":
        """spmvHipTriInfo: the schedule of that triangle (all zeros when it has not been analysed)."""
        info = spmvTriInfo()
        _check(lib.spmvHipTriInfo(C.byref(self.handle), SPMV_TRI_LOWER if lower else SPMV_TRI_UPPER, C.byref(info)),
               "spmvHipTriInfo")
        return info

    def solve_triangular(self, b, lower=True, unit_diagonal=False, out=None, sweeps=None):
        """hipSpTRSVCSR: x = T^-1 b for the lower (upper) triangle T of this square matrix, the other triangle ignored, with
        the bits of the serial loop (include/spmvHip.h).  b: a contiguous float64 device torch tensor of length N -> a torch
        tensor, `out` if given (same rules; `out` may be `b`: an in-place solve); or a numpy array -> uploaded, solved,
        returned as numpy.  Runs on the library stream.  sweeps=S: hipSpTRSVSweepsCSR, the iterate after S Jacobi sweeps on
        the triangle in place of the exact solution (its own loop in include/spmvHip.h; no level sets)."""
        N = int(self.handle.N)
        uplo = SPMV_TRI_LOWER if lower else SPMV_TRI_UPPER
        diag = SPMV_DIAG_UNIT if unit_diagonal else SPMV_DIAG_STORED
        with _Operands("solve_triangular", b) as ops:
            ops.vector("b", b, N)
            ops.result("out", out, (N,))
            if sweeps is None:
                _check(lib.hipSpTRSVCSR(C.byref(self.handle), uplo, diag, *ops.args), "hipSpTRSVCSR")
            else:
                _check(lib.hipSpTRSVSweepsCSR(C.byref(self.handle), uplo, diag, _sweep_count(sweeps), *ops.args), "hipSpTRSVSweepsCSR")
            return ops.value()

    def solve_triangular_block(self, B, lower=True, unit_diagonal=False, out=None, sweeps=None):
        """hipSpTRSMCSR: X = T^-1 B for a block of right-hand sides in one pass over the triangle, column c of X with the bits
        of solve_triangular on column c of B.  B is (N, k) float64: a device torch tensor with unit stride in one dimension
        (the rules of matmul's X) -> a torch tensor, `out` if given (same rules, its own layout; `out` may be `B`: an
        in-place solve); or a numpy array -> uploaded, solved, returned as numpy.  Runs on the library stream.  sweeps=S:
        hipSpTRSMSweepsCSR, column c with the bits of solve_triangular(..., sweeps=S) on column c."""
        N = int(self.handle.N)
        uplo = SPMV_TRI_LOWER if lower else SPMV_TRI_UPPER
        diag = SPMV_DIAG_UNIT if unit_diagonal else SPMV_DIAG_STORED
        with _Operands("solve_triangular_block", B) as ops:
            k, bl, ldb = ops.dense("B", B, N)
            xl, ldx = ops.result("out", out, (N, k))
            db, dx = ops.args
            if sweeps is None:
                _check(lib.hipSpTRSMCSR(C.byref(self.handle), uplo, diag, k, db, ldb, bl, dx, ldx, xl), "hipSpTRSMCSR")
            else:
                _check(lib.hipSpTRSMSweepsCSR(C.byref(self.handle), uplo, diag, _sweep_count(sweeps), k, db, ldb, bl, dx, ldx, xl),
                       "hipSpTRSMSweepsCSR")
            return ops.value()

    def prepare_triangular_sweeps(self, block_width=0):
        """spmvHipTriSweepsPrepare: build the plan of the sweep solves now, or widen its workspace to block_width columns
        (the first sweep solve does it otherwise)."""
        _check(lib.spmvHipTriSweepsPrepare(C.byref(self.handle), int(block_width)), "spmvHipTriSweepsPrepare")

    def set_triangular_apply(self, sweeps=None, block_width=0):
        """spmvHipTriSetApply: how cg, bicgstab, gmres, cg_block and bicgstab_block apply this handle as their preconditioner M.
        sweeps=None: the two exact triangular solves (the default).  sweeps=S or (S_lower, S_upper): that many Jacobi sweeps
        on each triangle, one launch per sweep and no level sets; block_width >= k is needed by the block solves.  Equal
        counts keep M^-1 symmetric (cg); unequal counts are for bicgstab and gmres."""
        if sweeps is None:
            _check(lib.spmvHipTriSetApply(C.byref(self.handle), SPMV_TRI_APPLY_EXACT, 0, 0, 0), "spmvHipTriSetApply")
            return
        lo, up = sweeps if isinstance(sweeps, (tuple, list)) else (sweeps, sweeps)
        _check(lib.spmvHipTriSetApply(C.byref(self.handle), SPMV_TRI_APPLY_SWEEPS, _sweep_count(lo), _sweep_count(up), int(block_width)),
               "spmvHipTriSetApply")

    def triangular_sweeps_info(self) -> "spmvTriSweepsInfo":
        """spmvHipTriSweepsInfo: the sweep plan of this handle (all zeros when it has none)."""
        info = spmvTriSweepsInfo()
        _check(lib.spmvHipTriSweepsInfo(C.byref(self.handle), C.byref(info)), "spmvHipTriSweepsInfo")
        return info

    def ilu0(self) -> "spmvIluInfo":
        """hipSpILU0CSR: overwrite this square matrix's values with its ILU(0) factors in place (L strictly lower with a unit
        diagonal, U the diagonal and above), with the bits of the serial loop (include/spmvHip.h); returns ilu0_info()."""
        _check(lib.hipSpILU0CSR(C.byref(self.handle)), "hipSpILU0CSR")
        return self.ilu0_info()

    def ilu0_info(self) -> "spmvIluInfo":
        """spmvHipIlu0Info: what the last factorisation of this matrix did (zeroPivot, firstBadRow, levels, ...)."""
        info = spmvIluInfo()
        _check(lib.spmvHipIlu0Info(C.byref(self.handle), C.byref(info)), "spmvHipIlu0Info")
        return info

    def fsai(self, pattern=None, lanes_per_row=0, storage="f64") -> "Fsai":
        """spmvHipFsaiSetup: the factorised sparse approximate inverse G of this square matrix, G^T G ~ A^-1, with the bits
        of the loop in include/spmvHip.h.  Only the lower triangle of this matrix is read.  pattern: a DeviceMatrix of the
        same size whose columns j < i give row i of G (its values are not read; it may be freed afterwards), None for this
        matrix's own; a row of G holds at most SPMV_FSAI_MAX_ROW entries.  lanes_per_row: 0 (the built-in choice), 4, 16
        or 64 -- no bit depends on it.  storage: "f32" applies the factor from single-precision storage (Fsai.set_storage).
        The result is accepted as `precond=` by cg / bicgstab / gmres / cg_block / bicgstab_block of any matrix of this size."""
        _storage(storage, "fsai")
        g = Fsai(self)
        opts = spmvFsaiOpts(int(lanes_per_row))
        _check(lib.spmvHipFsaiSetup(C.byref(self.handle), C.byref(pattern.handle) if pattern is not None else None, C.byref(opts),
                                    C.byref(g.handle), C.byref(g._info)), "spmvHipFsaiSetup")
        g.rows = int(g.handle.M)
        if storage != "f64":
            g.set_storage(storage)
        return g

    def cg(self, b, x0=None, precond=None, tol=1e-8, maxiter=1000, history=False):
        """hipSpCGCSR: solve A x = b (A symmetric positive definite) on the device with the bits of the loop in
        include/spmvHip.h; precond: None, a DeviceMatrix holding ILU(0) factors (`ilu0()`), this
        matrix's multigrid hierarchy (`amg()`) or an approximate-inverse factor (`fsai()`).  b (and x0): numpy arrays ->
        x as numpy; or contiguous float64 device torch tensors -> x as a new torch tensor.  Returns (x, info) with
        info.history a numpy array of the squared residuals hist[0 .. iterations] when history=True."""
        return self._krylov(lib.hipSpCGCSR, "hipSpCGCSR", b, x0, precond, tol, maxiter, history)

    def bicgstab(self, b, x0=None, precond=None, tol=1e-8, maxiter=1000, history=False):
        """hipSpBiCGStabCSR: solve A x = b (A square) by right-preconditioned BiCGStab; arguments and result as cg()."""
        return self._krylov(lib.hipSpBiCGStabCSR, "hipSpBiCGStabCSR", b, x0, precond, tol, maxiter, history)

    def gmres(self, b, x0=None, precond=None, tol=1e-8, maxiter=1000, restart=30, history=False):
        """hipSpGMRESCSR: solve A x = b (A square) by right-preconditioned restarted GMRES(restart) with CGS2; maxiter
        counts inner iterations over all cycles, 1 <= restart <= 64; the other arguments and the result as cg().
        info.history holds the estimates inside a cycle and the true squared residual at every cycle's last index."""
        return self._krylov(lib.hipSpGMRESCSR, "hipSpGMRESCSR", b, x0, precond, tol, maxiter, history, restart=restart)

    def eigsh(self, k=6, which="LA", ncv=None, v0=None, tol=1e-8, maxiter=None, keep=0, method="lanczos", precond=None):
        """The k algebraically largest (which="LA") or smallest ("SA") eigenpairs of this symmetric matrix, with the bits of
        the loops in include/spmvHip.h: method="lanczos" is hipSpLanczosCSR (thick-restart Lanczos), method="davidson"
        hipSpDavidsonCSR (generalised Davidson, k <= 16), which takes precond: None, or what cg() takes -- a DeviceMatrix
        holding ILU(0) factors, this matrix's multigrid hierarchy (`amg()`) or an approximate-inverse factor (`fsai()`) --,
        and then only which="SA".  Returns (theta, X, info): theta a numpy array of the info.found values in the order of
        the wanted end, X the (N, found) eigenvectors (numpy for a numpy v0, else a torch tensor with contiguous columns),
        info a spmvLanczosInfo or spmvDavidsonInfo with info.res the residual norms (Lanczos: estimates; Davidson:
        computed).  Conventions of this layer, not of the library: ncv=None means min(N, 64, max(2k + 1, 20)); v0=None
        means numpy.random.default_rng(0).standard_normal(N); maxiter=None means 10 N products A v."""
        N = int(self.handle.N)
        if which not in EIG_WHICH:
            raise SpmvHipError(f"eigsh: which must be one of {sorted(EIG_WHICH)}, not {which!r}")
        if method not in ("lanczos", "davidson"):
            raise SpmvHipError(f"eigsh: method must be 'lanczos' or 'davidson', not {method!r}")
        if precond is not None and method != "davidson":
            raise SpmvHipError("eigsh: precond is taken only by method='davidson'")
        if precond is not None and which != "SA":
            raise SpmvHipError("eigsh: precond is taken only with which='SA' (hipSpDavidsonCSR refuses it for the largest pairs)")
        k = int(k)
        ncv = min(N, 64, max(2 * k + 1, 20)) if ncv is None else int(ncv)
        if v0 is None:
            v0 = np.random.default_rng(0).standard_normal(N)
        davidson = method == "davidson"
        opts = (spmvDavidsonOpts if davidson else spmvLanczosOpts)(k, ncv, EIG_WHICH[which], float(tol),
                                                                 10 * N if maxiter is None else int(maxiter), int(keep))
        info = spmvDavidsonInfo() if davidson else spmvLanczosInfo()
        theta, res = np.zeros(max(k, 0)), np.zeros(max(k, 0))
        with _Operands("eigsh", v0) as ops:
            ops.vector("v0", v0, N)
            ops.result("X", None, (max(k, 0), N))                    # (row c of this block is column c of X: ldx = N)
            dv0, dx = ops.args
            if davidson:
                mh = C.byref(precond.handle) if precond is not None else None
                _check(lib.hipSpDavidsonCSR(C.byref(self.handle), mh, dv0, C.byref(opts), dx, N, _ptr(theta), _ptr(res), C.byref(info)),
                       "hipSpDavidsonCSR")
            else:
                _check(lib.hipSpLanczosCSR(C.byref(self.handle), dv0, C.byref(opts), dx, N, _ptr(theta), _ptr(res), C.byref(info)),
                       "hipSpLanczosCSR")
            X = ops.value()
        info.res = res[:info.found].copy()
        return theta[:info.found].copy(), X[:info.found].T, info

    def cg_block(self, B, X0=None, precond=None, tol=1e-8, maxiter=1000, history=False):
        """hipSpCGBlockCSR: k solves A x_c = b_c in lock step, column c of X with the bits of cg() on column c of B (and of
        X0), the matrix and the preconditioner's schedule streamed once per iteration for all columns.  B (and X0) are
        (N, k) float64: numpy arrays -> X as numpy; or device torch tensors with unit stride in one dimension (the rules
        of matmul's X) -> X as a new torch tensor.  precond: None, a DeviceMatrix holding ILU(0) factors, an approximate-inverse
        factor (`fsai()`), or this matrix's multigrid hierarchy after set_block_width(width >= k) (without one it is refused).  Returns (X, info): info.columns the k spmvKrylovColumn records; info.history, when
        history=True, a list of k arrays hist[0 .. iterations_c]."""
        return self._krylov_block(lib.hipSpCGBlockCSR, "hipSpCGBlockCSR", B, X0, precond, tol, maxiter, history)

    def bicgstab_block(self, B, X0=None, precond=None, tol=1e-8, maxiter=1000, history=False):
        """hipSpBiCGStabBlockCSR: as cg_block(), every column with the bits of bicgstab()."""
        return self._krylov_block(lib.hipSpBiCGStabBlockCSR, "hipSpBiCGStabBlockCSR", B, X0, precond, tol, maxiter, history)

    def _krylov_block(self, fn, name, B, X0, precond, tol, maxiter, history):
        N = int(self.handle.N)
        info = spmvKrylovInfo()
        mh = C.byref(precond.handle) if precond is not None else None
        with _Operands(name, B) as ops:
            k, bl, ldb = ops.dense("B", B, N)
            xl, ldx = ops.result("X", None, (N, k), init=("X0", X0))
            hist = np.zeros((k, int(maxiter) + 1), np.float64) if history else None
            opts = spmvKrylovOpts(float(tol), int(maxiter), hist.ctypes.data_as(C.POINTER(C.c_double)) if history else None)
            cols = (spmvKrylovColumn * k)()
            db, dx = ops.args
            _check(fn(C.byref(self.handle), mh, k, db, ldb, bl, dx, ldx, xl, C.byref(opts), cols, C.byref(info)), name)
            X = ops.value()
        info.columns = list(cols)
        if history:
            info.history = [hist[c, :cols[c].iterations + 1].copy() for c in range(k)]
        return X, info

    def _krylov(self, fn, name, b, x0, precond, tol, maxiter, history, restart=None):
        N = int(self.handle.N)
        hist = np.zeros(int(maxiter) + 1, np.float64) if history else None
        hp = hist.ctypes.data_as(C.POINTER(C.c_double)) if history else None
        if restart is None:
            opts = spmvKrylovOpts(float(tol), int(maxiter), hp)
        else:
            opts = spmvGmresOpts(float(tol), int(maxiter), int(restart), hp)
        info = spmvKrylovInfo()
        mh = C.byref(precond.handle) if precond is not None else None
        with _Operands(name, b) as ops:
            ops.vector("b", b, N)
            ops.result("x", None, (N,), init=("x0", x0))
            _check(fn(C.byref(self.handle), mh, *ops.args, C.byref(opts), C.byref(info)), name)
            x = ops.value()
        if history:
            info.history = hist[:info.iterations + 1].copy()
        return x, info

    def free(self):
        if self.handle.dev:
            lib.hipFreeSpmat(C.byref(self.handle))
        for k in self.keep:
            if hasattr(k, "free"):
                k.free()
        self.keep = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class AmgHierarchy(DeviceMatrix):
    """What DeviceMatrix.amg() returns: a hierarchy handle (no matrix: SpMV, formats and solves refuse it) with `info`
    (spmvAmgInfo), apply(), set_block_width(), block_info(), apply_block(), refresh_from(), level(), prolongator(), strength(), set_smoother(), smoother(), set_gauss_seidel(),
    gauss_seidel() and free().  It keeps a reference to its source matrix."""

    def __init__(self, source):
        super().__init__()
        self.source = source
        self.info = spmvAmgInfo()

    def apply(self, r, out=None):
        """spmvHipAmgApply: z = V(0, r), one cycle.  r: a numpy array -> z as numpy; or a float64 device torch tensor
        (any 8-byte alignment) -> z as a torch tensor (`out` when given)."""
        N = int(self.handle.M)
        with _Operands("spmvHipAmgApply", r) as ops:
            ops.vector("r", r, N)
            ops.result("out", out, (N,))
            _check(lib.spmvHipAmgApply(C.byref(self.handle), C.byref(self.source.handle), *ops.args), "spmvHipAmgApply")
            return ops.value()

    def set_block_width(self, width):
        """spmvHipAmgSetBlockWidth: the workspace of a block cycle for up to `width` columns (0 drops it); apply_block() and
        cg_block / bicgstab_block(precond=this hierarchy) then take up to that many.  Updates `info` (its bytes count it)."""
        _check(lib.spmvHipAmgSetBlockWidth(C.byref(self.handle), C.byref(self.source.handle), int(width)), "spmvHipAmgSetBlockWidth")
        _check(lib.spmvHipAmgInfo(C.byref(self.handle), C.byref(self.info)), "spmvHipAmgInfo")

    def set_storage(self, storage):
        """spmvHipAmgSetStorage: "f32" builds the single-precision value form on the source matrix, on every level's matrix and
        on every restriction and prolongator, and every product of the cycle (apply, apply_block, precond= of the solvers)
        streams 8 instead of 12 bytes per entry, arithmetic in double; "f64" (the state after a setup) releases them.
        refresh_from keeps the setting.  Refused on a hierarchy with a Gauss-Seidel level.  Returns the hierarchy, so that a
        setup chains: `A.amg(smoothed=True).set_storage("f32")`."""
        _check(lib.spmvHipAmgSetStorage(C.byref(self.handle), C.byref(self.source.handle), _storage(storage, "set_storage")), "spmvHipAmgSetStorage")
        return self

    def storage_info(self):
        """spmvHipAmgStorage as a dict: storage ('f64' or 'f32'), levels, f32_bytes (of the forms over all levels)."""
        v = spmvAmgStorageInfo()
        _check(lib.spmvHipAmgStorage(C.byref(self.handle), C.byref(v)), "spmvHipAmgStorage")
        return {"storage": "f32" if v.storage == SPMV_STORAGE_F32 else "f64", "levels": int(v.levels), "f32_bytes": int(v.f32Bytes)}

    def block_info(self):
        """spmvHipAmgBlock: the block workspace as a dict: width, bytes (zeros on a hierarchy without one)."""
        v = spmvAmgBlockInfo()
        _check(lib.spmvHipAmgBlock(C.byref(self.handle), C.byref(v)), "spmvHipAmgBlock")
        return {"width": int(v.width), "bytes": int(v.bytes)}

    def apply_block(self, R, out=None):
        """spmvHipAmgApplyBlock: Z(:, c) = V(0, R(:, c)), one cycle for all columns, column c with the bits of apply() on
        column c of R.  R is (M, k) float64 with k at most the width of set_block_width(): the operand rules of matmul (a
        device torch tensor with unit stride in one dimension -> a torch tensor, `out` if given; or a numpy array -> numpy)."""
        N = int(self.handle.M)
        with _Operands("spmvHipAmgApplyBlock", R) as ops:
            k, rl, ldr = ops.dense("R", R, N)
            zl, ldz = ops.result("out", out, (N, k))
            dr, dz = ops.args
            _check(lib.spmvHipAmgApplyBlock(C.byref(self.handle), C.byref(self.source.handle), k, dr, ldr, rl, dz, ldz, zl),
                   "spmvHipAmgApplyBlock")
            return ops.value()

    def refresh_from(self, source: "DeviceMatrix"):
        """spmvHipAmgRefresh: `source` (the matrix of the setup) has new values on the same pattern."""
        _check(lib.spmvHipAmgRefresh(C.byref(self.handle), C.byref(source.handle)), "spmvHipAmgRefresh")
        _check(lib.spmvHipAmgInfo(C.byref(self.handle), C.byref(self.info)), "spmvHipAmgInfo")

    def level(self, l):
        """spmvHipAmgLevel: (view, agg, dinv) of level l: an spmat copy whose arrays stay the hierarchy's (dev = NULL), and
        the device addresses of agg_l (None on the last level) and dinv_l"""
        view, agg, dinv = spmat(), C.c_void_p(), C.c_void_p()
        _check(lib.spmvHipAmgLevel(C.byref(self.handle), int(l), C.byref(view), C.byref(agg), C.byref(dinv)), "spmvHipAmgLevel")
        return view, agg.value, dinv.value

    def prolongator(self, l):
        """spmvHipAmgProlongator: (P, R, omegaP) of level l (not the last): P_l and R_l as host CSR arrays (M, N, IRP, JA,
        AS), downloaded, and the damping w_l (0.0 on a hierarchy that is not smoothed)"""
        P, R, w = spmat(), spmat(), C.c_double()
        _check(lib.spmvHipAmgProlongator(C.byref(self.handle), int(l), C.byref(P), C.byref(R), C.byref(w)), "spmvHipAmgProlongator")
        return self._down(P), self._down(R), w.value

    @staticmethod
    def _down(v):
        """the host CSR arrays (M, N, IRP, JA, AS) of a view"""
        M, NZ = int(v.M), int(v.NZ)
        out = [np.empty(M + 1, np.uint32), np.empty(NZ, np.uint32), np.empty(NZ, np.float64)]
        for a, ptr in zip(out, (v.IRP, v.JA, v.AS)):
            if a.size:
                _check(lib.spmvHipMemcpyDown(a.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), a.nbytes), "spmvHipMemcpyDown")
        return M, int(v.N), out[0], out[1], out[2]

    def strength(self, l):
        """spmvHipAmgStrength: (F, theta) of level l (not the last) of a hierarchy made with theta / thetaScale: the
        strength-filtered F_l as host CSR arrays (M, N, IRP, JA, AS), downloaded, and its threshold theta_l"""
        F, theta = spmat(), C.c_double()
        _check(lib.spmvHipAmgStrength(C.byref(self.handle), int(l), C.byref(F), C.byref(theta)), "spmvHipAmgStrength")
        return self._down(F), theta.value

    def set_smoother(self, kind="chebyshev", nu1=None, nu2=None, nuCoarse=None, eig_ratio=None, lambda_scale=None):
        """spmvHipAmgSetSmoother: what the cycle smooths with from now on, "jacobi" or "chebyshev" (or the header's number),
        and how often: a count None keeps the hierarchy's, 0 asks for none.  eig_ratio (10) and lambda_scale (1.0) are the
        Chebyshev interval: lambda_max = lambda_scale * rho_l, lambda_min = lambda_max / eig_ratio.  A cycle captured
        earlier must be captured again.  `info` is read again (its bytes count the coefficient tables)."""
        kinds = {"jacobi": SPMV_AMG_SMOOTHER_JACOBI, "chebyshev": SPMV_AMG_SMOOTHER_CHEBYSHEV}
        if isinstance(kind, str) and kind not in kinds:
            raise SpmvHipError(f"set_smoother: kind {kind!r} is neither 'jacobi' nor 'chebyshev'")
        opts = spmvAmgSmootherOpts(kinds[kind] if isinstance(kind, str) else int(kind), _amg_sweeps(nu1), _amg_sweeps(nu2), _amg_sweeps(nuCoarse),
                                   float(eig_ratio or 0.0), float(lambda_scale or 0.0))
        _check(lib.spmvHipAmgSetSmoother(C.byref(self.handle), C.byref(self.source.handle), C.byref(opts)), "spmvHipAmgSetSmoother")
        _check(lib.spmvHipAmgInfo(C.byref(self.handle), C.byref(self.info)), "spmvHipAmgInfo")

    def smoother(self, l):
        """spmvHipAmgSmoother: the smoother of level l as a dict: kind, nu1, nu2, nuCoarse (the counts in force), rho,
        lambdaMax, lambdaMin, dCoef (the device address of the table, None without one) and coef, the table downloaded: an
        (nCoef, 2) array of the pairs (a_k, b_k)"""
        v = spmvAmgSmootherInfo()
        _check(lib.spmvHipAmgSmoother(C.byref(self.handle), int(l), C.byref(v)), "spmvHipAmgSmoother")
        coef = np.empty((int(v.nCoef), 2), np.float64)
        if coef.size:
            _check(lib.spmvHipMemcpyDown(coef.ctypes.data_as(C.c_void_p), C.cast(v.dCoef, C.c_void_p), coef.nbytes), "spmvHipMemcpyDown")
        return dict(kind=int(v.kind), nu1=int(v.nu1), nu2=int(v.nu2), nuCoarse=int(v.nuCoarse), rho=float(v.rho), lambdaMax=float(v.lambdaMax),
                    lambdaMin=float(v.lambdaMin), dCoef=C.cast(v.dCoef, C.c_void_p).value, coef=coef)

    def set_gauss_seidel(self, omega=None, order="natural", seed=0, one_way=False, levels=None, nu1=None, nu2=None, nuCoarse=None):
        """spmvHipAmgSetGaussSeidel: the cycle smooths with multicolour Gauss-Seidel sweeps from now on.  omega: the
        relaxation (1.0); order / seed: those of the colouring ("natural" or "hash", or the header's number); one_way:
        forward everywhere instead of forward before and backward after the correction; levels: Gauss-Seidel on the levels
        below it, damped Jacobi from it on (None: all); a count None keeps the hierarchy's, 0 asks for none.  A cycle captured
        earlier must be captured again.  `info` is read again (its bytes count the colour lists)."""
        if isinstance(order, str) and order not in COLOUR_ORDERS:
            raise SpmvHipError(f"set_gauss_seidel: order {order!r} is neither 'natural' nor 'hash'")
        opts = spmvAmgGsOpts(COLOUR_ORDERS[order] if isinstance(order, str) else int(order), int(seed) & 0xFFFFFFFF, float(omega or 0.0),
                             int(bool(one_way)), int(levels or 0), _amg_sweeps(nu1), _amg_sweeps(nu2), _amg_sweeps(nuCoarse))
        _check(lib.spmvHipAmgSetGaussSeidel(C.byref(self.handle), C.byref(self.source.handle), C.byref(opts)), "spmvHipAmgSetGaussSeidel")
        _check(lib.spmvHipAmgInfo(C.byref(self.handle), C.byref(self.info)), "spmvHipAmgInfo")

    def gauss_seidel(self, l):
        """spmvHipAmgGaussSeidel: the Gauss-Seidel state of level l as a dict: active, colours, maxColourRows, longRows,
        small, omega, order, seed, oneWay, dPerm / dColourPtr (device addresses, None on a level that does not sweep by
        colours) and perm / colourPtr, the two lists downloaded (None likewise)"""
        v = spmvAmgGsInfo()
        _check(lib.spmvHipAmgGaussSeidel(C.byref(self.handle), int(l), C.byref(v)), "spmvHipAmgGaussSeidel")
        out = dict(active=int(v.active), colours=int(v.colours), maxColourRows=int(v.maxColourRows), longRows=int(v.longRows), small=int(v.small),
                   omega=float(v.omega), order=int(v.order), seed=int(v.seed), oneWay=int(v.oneWay), dPerm=C.cast(v.dPerm, C.c_void_p).value,
                   dColourPtr=C.cast(v.dColourPtr, C.c_void_p).value, perm=None, colourPtr=None)
        if v.active:
            view = spmat()
            _check(lib.spmvHipAmgLevel(C.byref(self.handle), int(l), C.byref(view), None, None), "spmvHipAmgLevel")
            out["perm"], out["colourPtr"] = np.empty(int(view.M), np.uint32), np.empty(int(v.colours) + 1, np.uint32)
            for a, ptr in ((out["perm"], v.dPerm), (out["colourPtr"], v.dColourPtr)):
                if a.size:
                    _check(lib.spmvHipMemcpyDown(a.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), a.nbytes), "spmvHipMemcpyDown")
        return out

    def free(self):
        super().free()
        self.source = None


class Fsai(DeviceMatrix):
    """What DeviceMatrix.fsai() returns: the factor G as an ordinary CSR DeviceMatrix (SpMV, transpose, multiply, filter and
    to_coo take it) that privately owns G^T and the workspace of apply(); free() gives all of it back.  It keeps a reference
    to its source matrix."""

    def __init__(self, source):
        super().__init__()
        self.source = source
        self._info = spmvFsaiInfo()

    def apply(self, r, out=None):
        """spmvHipFsaiApply: z = G^T (G r), two serial-order SpMVs.  r: a numpy array -> z as numpy; or a float64 device
        torch tensor -> z as a torch tensor (`out` when given; `out` may be `r`: in place)."""
        N = int(self.handle.M)
        with _Operands("spmvHipFsaiApply", r) as ops:
            ops.vector("r", r, N)
            ops.result("out", out, (N,))
            _check(lib.spmvHipFsaiApply(C.byref(self.handle), *ops.args), "spmvHipFsaiApply")
            return ops.value()

    def refresh_from(self, source: "DeviceMatrix"):
        """spmvHipFsaiRefresh: `source` (the matrix of the setup) has new values on the same pattern: G and G^T take the
        values of a fresh setup in place, addresses kept.  Returns info()."""
        _check(lib.spmvHipFsaiRefresh(C.byref(self.handle), C.byref(source.handle), C.byref(self._info)), "spmvHipFsaiRefresh")
        return self._info

    def set_storage(self, storage):
        """spmvHipFsaiSetStorage: "f32" builds the single-precision value form on G and on the factor's G^T, and every
        application (apply, precond= of the solvers) becomes two f32 products -- 8 instead of 12 bytes per entry streamed,
        arithmetic in double; "f64" (the state after a setup) releases them.  refresh_from keeps the setting."""
        _check(lib.spmvHipFsaiSetStorage(C.byref(self.handle), _storage(storage, "set_storage")), "spmvHipFsaiSetStorage")

    @property
    def storage(self):
        """spmvHipFsaiStorage: the setting, 'f64' or 'f32'"""
        s = _i(0)
        _check(lib.spmvHipFsaiStorage(C.byref(self.handle), C.byref(s)), "spmvHipFsaiStorage")
        return "f32" if s.value == SPMV_STORAGE_F32 else "f64"

    def transposed(self):
        """spmvHipFsaiTranspose: the G^T this factor owns as host CSR arrays (M, N, IRP, JA, AS), downloaded"""
        view = spmat()
        _check(lib.spmvHipFsaiTranspose(C.byref(self.handle), C.byref(view)), "spmvHipFsaiTranspose")
        return AmgHierarchy._down(view)

    def info(self) -> "spmvFsaiInfo":
        """spmvHipFsaiInfo: what the setup or the last refresh did (nnz, maxRow, badRows, firstBadRow, ...)."""
        _check(lib.spmvHipFsaiInfo(C.byref(self.handle), C.byref(self._info)), "spmvHipFsaiInfo")
        return self._info

    def free(self):
        super().free()
        self.source = None


class Colouring:
    """What DeviceMatrix.colour() returns: the device arrays `perm` and `colours` (None unless asked for) and `info`."""

    def __init__(self, perm, colours, info):
        self.perm, self.colours, self.info = perm, colours, info

    def free(self):
        for b in (self.perm, self.colours):
            if isinstance(b, DeviceBuffer):
                b.free()
        self.perm = self.colours = None


class Ordering:
    """What DeviceMatrix.rcm() returns: the device array `perm` and `info`."""

    def __init__(self, perm, info):
        self.perm, self.info = perm, info

    def free(self):
        if isinstance(self.perm, DeviceBuffer):
            self.perm.free()
        self.perm = None


def _dev_ptr(b):
    """the device address of a DeviceBuffer or a torch tensor (None stays None)"""
    if b is None:
        return None
    return b.ptr if isinstance(b, DeviceBuffer) else C.c_void_p(b.data_ptr())


def _perm_len(perm, who):
    """entries of a device permutation: a DeviceBuffer of uint32, or an int32 tensor under the 1-D rule of a device call"""
    return perm.nbytes // 4 if isinstance(perm, DeviceBuffer) else _device_vector(who, "perm", perm, int32=True)


def permute_vector(perm, v, inverse=False, out=None):
    """spmvHipVecPermute: forward out[r] = v[perm[r]] (b' = P b), inverse out[perm[r]] = v[r] (x = P^T x'); bits are copied.
    perm: a Colouring, an Ordering, a DeviceBuffer of uint32 or an int32 device torch tensor.  v: a 1-D float64 device torch
    tensor with unit stride (any element offset) -> a torch tensor, `out` if given (same rules, not v itself); or a numpy
    array -> uploaded, permuted, returned as numpy.  Runs on the library stream."""
    perm = perm.perm if isinstance(perm, (Colouring, Ordering)) else perm
    n = _perm_len(perm, "permute_vector")
    with _Operands("permute_vector", v) as ops:
        ops.vector("v", v, n)
        ops.result("out", out, (n,))
        _check(lib.spmvHipVecPermute(n, _dev_ptr(perm), *ops.args, 1 if inverse else 0), "spmvHipVecPermute")
        return ops.value()


def _dense_layout(t, what, who="matmul"):
    """(layout, leading dimension) of a 2-D float64 device tensor of shape (rows, k) with unit stride in one dimension"""
    torch = _torch()
    if t.dtype != torch.float64 or not t.is_cuda:
        raise SpmvHipError(f"{who}: {what} must be a float64 tensor on the device")
    (rows, k), (s0, s1) = t.shape, t.stride()
    if (s1 == 1 or k == 1) and s0 >= k:
        return SPMV_DENSE_ROW_MAJOR, s0
    if (s0 == 1 or rows == 1) and s1 >= rows:
        return SPMV_DENSE_COL_MAJOR, s1
    raise SpmvHipError(f"{who}: {what} needs unit stride in one dimension (strides {t.stride()})")


def spMatCpyCSR(host: HostCSR) -> DeviceMatrix:
    d = DeviceMatrix()
    _check(lib.spMatCpyCSR(C.byref(host.struct), C.byref(d.handle)), "spMatCpyCSR")
    d.rows = host.M
    return d


def assemble_coo(M, N, rows, cols, vals, duplicates="sum", keep_map=True) -> DeviceMatrix:
    """spmvHipCooAssemble: the M x N CSR matrix assembled on the device from the triplets (rows[e], cols[e], vals[e]), as a new
    DeviceMatrix that owns its handle, bit for bit the serial loop of include/spmvHip.h: rows ascending, the duplicates of an
    (i, j) added in input order ("sum") or the last one taken ("last"), an entry whose row or column is the skip marker
    left out.  The three operands are numpy arrays -- index arrays of any integer dtype, -1 or 2^32 - 1 the skip marker,
    range-checked and uploaded as uint32 for the call -- or device torch tensors (int32, int32, float64: -1 the skip marker),
    used in place without a copy.  keep_map: keep what assemble_refresh() needs.  assemble_info() tells what the call did."""
    if isinstance(duplicates, str) and duplicates not in COO_DUPLICATES:
        raise SpmvHipError(f"assemble_coo: duplicates must be one of {sorted(COO_DUPLICATES)}, not {duplicates!r}")
    opts = spmvCooOpts(COO_DUPLICATES[duplicates] if isinstance(duplicates, str) else int(duplicates), int(bool(keep_map)))
    c, info = DeviceMatrix(), spmvCooInfo()
    with _Operands("assemble_coo", rows) as ops:
        n = ops.triplets("rows", rows, index=True)
        ops.triplets("cols", cols, n, index=True)
        ops.triplets("vals", vals, n)
        _check(lib.spmvHipCooAssemble(int(M), int(N), n, *ops.args, C.byref(opts), C.byref(c.handle), C.byref(info)), "spmvHipCooAssemble")
    c.rows = int(c.handle.M)
    c._coo = info
    return c


def spMatCpyELL(host: HostELL) -> DeviceMatrix:
    d = DeviceMatrix()
    _check(lib.spMatCpyELL(C.byref(host.struct), C.byref(d.handle)), "spMatCpyELL")
    d.rows = host.rows
    return d


def csr_to_ell_device(dcsr: DeviceMatrix, transposed: bool) -> DeviceMatrix:
    d = DeviceMatrix()
    _check(lib.spmvHipCsrToEll(C.byref(dcsr.handle), 1 if transposed else 0, C.byref(d.handle)), "spmvHipCsrToEll")
    d.rows = dcsr.rows
    return d


def spmv(launcher: str, dmat: DeviceMatrix, dx: DeviceVector, dy: DeviceVector, cfg: CONFIG = None):
    """Run one of the five HIP launchers; raises on EXIT_FAILURE."""
    fn = SPMV_LAUNCHERS[launcher]
    _check(fn(C.byref(dmat.handle), dx.ptr, cfg if cfg is not None else CONFIG(), dy.ptr), launcher)


def build_tiles(dmat: DeviceMatrix, rowsPerBin=0, taper=False, ntStore=-1, chunk=0, deterministic=False):
    """spmvHipBuildTilesOpt: (re)build the two-phase format of this handle with explicit options."""
    o = spmvTilesOpts(int(rowsPerBin), 1 if taper else 0, int(ntStore), int(chunk), 1 if deterministic else 0)     # (no second form for this format)
    _check(lib.spmvHipBuildTilesOpt(C.byref(dmat.handle), C.byref(o)), "spmvHipBuildTilesOpt")


def tiles_info(dmat: DeviceMatrix) -> spmvTilesInfo:
    info = spmvTilesInfo()
    _check(lib.spmvHipTilesInfo(C.byref(dmat.handle), C.byref(info)), "spmvHipTilesInfo")
    return info


def build_stripes(dmat: DeviceMatrix, rowsPerBin=0, grid=0, spread=-1, wide=-1, deterministic=False):
    """spmvHipBuildStripesOpt: (re)build the stripes format of this handle with explicit options."""
    o = spmvStripesOpts(int(rowsPerBin), int(grid), int(spread), int(wide), int(deterministic))
    _check(lib.spmvHipBuildStripesOpt(C.byref(dmat.handle), C.byref(o)), "spmvHipBuildStripesOpt")


def stripes_info(dmat: DeviceMatrix) -> spmvStripesInfo:
    info = spmvStripesInfo()
    _check(lib.spmvHipStripesInfo(C.byref(dmat.handle), C.byref(info)), "spmvHipStripesInfo")
    return info


def dot(u, v):
    """spmvHipDot: u . v of two float64 device torch tensors of one length (1-D, unit stride; any element offset) in the
    fixed order of include/spmvHip.h, as a 0-d float64 tensor on the same device.  Runs on the library stream."""
    with _Operands("dot", u, host_calls=False) as ops:
        n = ops.vector("u", u)
        ops.vector("v", v, n)
        ops.result("out", None, ())
        _check(lib.spmvHipDot(n, *ops.args), "spmvHipDot")
        return ops.value()


def multi_dot(V, w):
    """spmvHipMultiDot: h = V^T w, every h[i] the bits of dot(V[:, i], w).  V: a 2-D float64 device torch tensor (n, k) whose
    columns are contiguous (V.stride(0) == 1, ldv = V.stride(1) >= n) and w a 1-D one of length n with unit stride -> a
    length-k device tensor; or numpy arrays (V in Fortran order, else copied to it) -> a numpy array."""
    with _Operands("multi_dot", V) as ops:
        n, k, ldv = ops.columns("V", V)
        ops.vector("w", w, n, least=8)
        ops.result("h", None, (k,), least=8)
        dV, dw, dh = ops.args
        _check(lib.spmvHipMultiDot(n, k, dV, ldv, dw, dh), "spmvHipMultiDot")
        return ops.value()


def block_combine(V, S):
    """spmvHipBlockCombine: Y = V S with Y[i, c] the sum of V[i, j] * S[j, c] over ascending j from +0.0, every product and
    every add rounded on its own.  V (n, m) and S (m, k), m and k in 1 .. 64: 2-D float64 device torch tensors with
    contiguous columns (the rule of multi_dot's V) -> an (n, k) device tensor with contiguous columns; or numpy arrays ->
    a numpy array."""
    with _Operands("block_combine", V) as ops:
        n, m, ldv = ops.columns("V", V)
        ms, k, lds = ops.columns("S", S)
        if ms != m:
            raise SpmvHipError(f"block_combine: S must have {m} rows, not {ms}")
        ops.result("Y", None, (k, n), least=8)                       # (row c of this block is column c of Y: ldy = n)
        dV, dS, dY = ops.args
        _check(lib.spmvHipBlockCombine(n, m, k, dV, ldv, dS, max(lds, m), dY, max(n, 1)), "spmvHipBlockCombine")
        return ops.value().T


def block_residual(V, W, S, theta):
    """spmvHipBlockResidual: (R, norm2) with R[i, c] = (sum_j W[i, j] S[j, c]) - theta[c] * (sum_j V[i, j] S[j, c]), both sums over
    ascending j from +0.0 with every product and add rounded on its own, and norm2[c] the bits of dot(R[:, c], R[:, c]).  V and
    W (n, m), S (m, k), theta (k,), m in 1 .. 64, k in 1 .. 16: float64 device torch tensors, the 2-D ones with contiguous
    columns (the rule of multi_dot's V) -> R an (n, k) device tensor with contiguous columns and norm2 a length-k one (two
    views of one new tensor); or numpy arrays -> numpy arrays."""
    with _Operands("block_residual", V) as ops:
        n, m, ldv = ops.columns("V", V)
        nw, mw, ldw = ops.columns("W", W)
        ms, k, lds = ops.columns("S", S)
        if (nw, mw) != (n, m) or ms != m:
            raise SpmvHipError(f"block_residual: W must be ({n}, {m}) and S must have {m} rows, not {(nw, mw)} and {ms}")
        ops.vector("theta", theta, k, least=8)
        ops.result("R", None, (k * n + k,), least=8)                 # (column c of R at [c*n ..]: ldr = n; then norm2)
        dV, dW, dS, dTheta, dR = ops.args
        _check(lib.spmvHipBlockResidual(n, m, k, dV, ldv, dW, max(ldw, n, 1), dS, max(lds, m), dTheta, dR, max(n, 1), dR + 8 * k * n),
               "spmvHipBlockResidual")
        out = ops.value()
        return out[:k * n].reshape(k, n).T, out[k * n:]


def block_dot(U, V):
    """spmvHipBlockDot: h[c] = U[:, c] . V[:, c], every h[c] the bits of dot(U[:, c], V[:, c]).  U and V are (n, k) float64
    with k >= 1: device torch tensors with unit stride in one dimension, each in its own layout (the rules of matmul's
    X; V may be U) -> a length-k device tensor; or numpy arrays -> a numpy array."""
    with _Operands("block_dot", U) as ops:
        k, ul, ldu = ops.dense("U", U, U.shape[0] if U.ndim == 2 else -1)
        kv, vl, ldv = ops.dense("V", V, U.shape[0])
        if kv != k:
            raise SpmvHipError(f"block_dot: V must have {k} columns, not {kv}")
        ops.result("h", None, (k,), least=8)
        dU, dV, dh = ops.args
        _check(lib.spmvHipBlockDot(U.shape[0], k, dU, ldu, ul, dV, ldv, vl, dh), "spmvHipBlockDot")
        return ops.value()


def set_variant(launcher: str, variant: int):
    _check(lib.spmvHipSetVariant(launcher.encode(), int(variant)), "spmvHipSetVariant")


def last_launch():
    g, b = spmvDim3(), spmvDim3()
    lib.spmvHipLastLaunch(C.byref(g), C.byref(b))
    return (g.x, g.y, g.z), (b.x, b.y, b.z)


def partition_rows(IRP, n_parts):
    IRP = np.ascontiguousarray(IRP, dtype=np.uint64)
    bounds = np.zeros(n_parts + 1, dtype=np.uint64)
    _check(lib.spmvHipPartitionRows(_ptr(IRP), IRP.size - 1, n_parts, _ptr(bounds)), "spmvHipPartitionRows")
    return bounds
