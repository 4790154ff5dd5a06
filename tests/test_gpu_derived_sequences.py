"""Seeded operation sequences on a graph of DERIVED device handles, checked step by step against a host model.

tests/test_gpu_sequences.py keeps using uploaded handles the way an iterative caller does; this module does the same for
the handles that are made from other handles -- transposes, permutations by a colouring, products, sums and filters, up to
five deep -- whose refreshes, ILU(0) in place and direct value updates all end in the one value-update tail of the library.
tests/derived_model.py holds the model and the generator (every draw from the seed and the model alone, so
tests/test_derived_model.py runs the same traces without a GPU and checks what they cover); this file executes each
record on the device:
  * after every operation that writes a node its IRP, JA and AS come back and are the model's bits (a NaN only has to be a
    NaN), spmvHipUnitValue is the model's unit flag and value, spmvHipLastUpdateInfo what the model of the tail expects,
    and both kernel selections are forgotten exactly when the values stopped being unit;
  * a stale node keeps its old values; a refresh from a wrong, freed or re-uploaded source (or a pair in the other order)
    is refused on the host and leaves the node's bytes alone; a node whose source was freed keeps working;
  * every product launcher and matmul (k = 1, 3, 16) on the nodes: serial-order paths as bits, any-order paths by
    exact_ref.check_any_order and tight_error <= 1e-13, y poisoned first;
  * triangular solves (single and block) against trsv_ref / trsm_ref; ilu0() in place against ilu0_ref with its zero-pivot
    report, L and U solves on the factors, the unfactored bits back after the next refresh;
  * cg / bicgstab / gmres with no preconditioner or a factored copy: x, status and iteration count of the reference loops;
  * multigrid hierarchies (plain, smoothed, strength) on the square nodes: set_smoother, set_gauss_seidel, set_block_width
    and refresh_from in random order, every step followed by one cycle (and a block cycle where a workspace stands) with
    the bits of the amg_*_ref cycle for the settings in force; apply() also against a twin set up fresh with the same
    settings; a block cycle wider than the workspace or on a Gauss-Seidel hierarchy is refused and changes nothing.
A step whose result the model marks as unspecified (tests/test_derived_model.py caps them at a tenth per kind) is skipped;
an unexpected refusal is a failure.
Every failure names the seed and the whole trace up to the failing step; one seed runs alone by its id
(tests/test_gpu_derived_sequences.py::test_derived_sequence[7]).

20 seeds of 50 operations each, plus the uploads, a final cycle of every live hierarchy and a final serial-order product on
every live node; measured on one MI355X: 19 s for the module, 11 s of them the first test's start of the runtime (1 250
operations; 291 checked products, 132 triangular solves, 28 Krylov solves, 248 cycles, 785 downloads of a node's arrays)."""
import pytest

import derived_model as dm
from derived_device import MEM_TOL, Device, api, stream, torch  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


_memory = {}


@pytest.mark.parametrize("seed", dm.SEEDS)
def test_derived_sequence(api, torch, oracle, stream, seed):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    gen = dm.Generator(seed)
    dev = Device(api, torch, oracle, gen, stream)
    try:
        for rec in gen.run():
            dev.execute(rec)
        c = dev.counts
        print(f"seed {seed}: {len(gen.trace)} operations, {c['products']} checked products, {c['solves']} solves, "
              f"{c['krylov']} Krylov solves, {c['cycles']} cycles, {c['downloads']} node downloads")
    finally:
        api.lib.spmvHipDeviceSynchronize()
        for h in dev.hh.values():
            h.free()
        dev.hh.clear()
        for d in dev.h.values():
            d.free()
        dev.h.clear()
        dev.adopted.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1 = torch.cuda.mem_get_info()[0]
    # the first seed of the process may load code objects and the library's shared workspace: from the second seed on
    # free memory must come back to where the first one left it
    assert free1 >= free0 - (256 << 20), (seed, free0, free1)
    base = _memory.setdefault("after first seed", free1)
    assert free1 >= base - MEM_TOL, f"seed {seed}: {(base - free1) >> 20} MiB not given back"
