"""The Python mirror of include/spmvHip.h agrees with the header, taken from the header itself: every struct typedef is a
ctypes.Structure in spmv_openmp_cuda_amd.api with the header's field names in the header's order, the size gcc gives it and
every field at gcc's offset; and every prototype is bound in api._sigs with as many argtypes as it has parameters.
No GPU needed."""
import ctypes as C

import pytest

import c_header

STRUCTS = c_header.structs()
PROTOTYPES = c_header.prototypes()


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    return a


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{struct: [sizeof, offsetof of every field]} from one C program over every struct of the header"""
    body = ""
    for name, fields in STRUCTS.items():
        body += f'    printf("{name} %zu", sizeof({name}));\n'
        body += "".join(f'    printf(" %zu", offsetof({name}, {f}));\n' for f in fields) + '    printf("\\n");\n'
    lines = c_header.run_c(tmp_path_factory.mktemp("layout"), body, "layout").splitlines()
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in lines}


def test_the_header_and_the_mirror_hold_the_same_structs(api):
    mirrored = {n for n, v in vars(api).items() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == api.__name__}
    assert len(STRUCTS) >= 18
    assert mirrored == set(STRUCTS)


@pytest.mark.parametrize("struct", list(STRUCTS))
def test_struct_layout_matches_c(api, c_layout, struct):
    py = getattr(api, struct)
    fields = [f[0] for f in py._fields_]
    assert fields == STRUCTS[struct], "field names and their order"
    assert c_layout[struct] == [C.sizeof(py)] + [getattr(py, f).offset for f in fields]


def test_every_prototype_is_bound_with_its_parameter_count(api):
    assert len(PROTOTYPES) >= 103
    unbound = sorted(set(PROTOTYPES) - set(api._sigs))
    assert not unbound, f"declared in include/spmvHip.h, missing from api._sigs: {unbound}"
    wrong = {n: (len(api._sigs[n][0]), k) for n, k in PROTOTYPES.items() if len(api._sigs[n][0]) != k}
    assert not wrong, f"(argtypes, parameters of the prototype): {wrong}"
    for n, k in PROTOTYPES.items():
        assert len(getattr(api.lib, n).argtypes) == k, n
