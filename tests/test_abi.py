"""CPU tests of the C-ABI boundary: the library builds for gfx950, loads,
and exports exactly what include/vrpms.h declares (no compute calls), and
vrpms_set_option's validator -- its refusals on the CPU, its accepted values
in one test on the GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrpms.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vrpms_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def libpath():
    from vrpms_amd.build import build_library
    return build_library()


def test_library_is_gfx950(libpath):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-S", libpath],
                         capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    blob = open(libpath, "rb").read()
    assert b"gfx950" in blob


def test_exports_every_declared_symbol(libpath):
    import torch  # noqa: F401 -- same load order as the product binding
    lib = ctypes.CDLL(libpath)
    decl = declared_functions()
    assert len(decl) >= 8
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in vrpms.h but not exported"


def test_ctypes_signatures_cover_header():
    from vrpms_amd._lib import SIGNATURES
    assert sorted(SIGNATURES) == declared_functions()


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "vrpms.h"\nint main(void){return vrpms_version() < 0;}\n')
    res = subprocess.run(["gcc", "-c", "-std=c99", "-Wall", "-Werror", "-I",
                          os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_version_and_error_paths_without_gpu(libpath):
    import torch  # noqa: F401
    lib = ctypes.CDLL(libpath)
    lib.vrpms_version.restype = ctypes.c_int
    assert lib.vrpms_version() >= 1
    # NULL ctx is rejected before any HIP call
    lib.vrpms_eval.restype = ctypes.c_int
    assert lib.vrpms_eval(None, None, 1, 0, 0, 0, None, None, None, None, None) == -1
    lib.vrpms_last_error.restype = ctypes.c_char_p
    assert b"ctx is NULL" in lib.vrpms_last_error()


# vrpms_set_option's validator (capi.hip): option -> (wording of its refusal,
# accepted values, refused values: one below, one above and any gap inside)
OPTIONS = {
    1: (b"split mode", (0, 2, 3), (-1, 1, 4)),
    2: (b"staged M", (0, 1, 2), (-1, 3)),
    3: (b"words kernel", (0, 1), (-1, 2)),
    4: (b"words ILP", (0, 2), (-1, 1, 3)),          # 1 only in -DVRPMS_AB builds
    5: (b"words lookahead", (0, 1, 2), (-1, 3)),
    6: (b"rows config", (0, 1, 2, 3, 4, 5), (-1, 6)),
    7: (b"GA fused", (0, 2), (-1, 1, 3)),
    8: (b"SA route", (0, 2, 3, 4), (-1, 1, 5)),
    9: (b"route workgroups per CU", (0, 1, 2), (-1, 3)),
    10: (b"island timeout", (1, 120, 2**31 - 1), (0, -1, -2**31)),   # any value > 0
    11: (b"segment-kernel wavefronts", (0, 1, 2, 3, 4), (-1, 5)),
    12: (b"ACO construct", (0, 2), (-1, 1, 3)),
    13: (b"batch DP team", (0, 16, 32, 64, 128, 256), (-1, 8, 48, 255, 512)),
}
OPTION_DEFAULT = {10: 120}


def test_option_table_covers_the_header():
    from vrpms_amd import _lib
    text = open(HEADER).read()
    numbers = {name: int(v) for name, v in re.findall(r"#define (VRPMS_OPT_[A-Z_]+) (\d+)", text)}
    assert sorted(numbers.values()) == sorted(OPTIONS)
    assert {getattr(_lib, k[len("VRPMS_"):]) for k in numbers} == set(OPTIONS)


def test_set_option_refusals_need_no_gpu(libpath):
    """A refusal comes before the context is written, so a block of zeros
    stands in for the non-NULL ctx, and stays zero."""
    from vrpms_amd import _lib
    lib = _lib.load()
    f = lib.vrpms_set_option
    fake = ctypes.create_string_buffer(1 << 16)
    c = ctypes.addressof(fake)
    assert f(None, 2, 1) == _lib.VRPMS_EINVAL
    assert b"vrpms_set_option" in lib.vrpms_last_error() and b"ctx is NULL" in lib.vrpms_last_error()
    for opt in (0, 14, -1, 2**31 - 1):
        assert f(c, opt, 0) == _lib.VRPMS_EINVAL
        assert b"vrpms_set_option: unknown option %d" % opt in lib.vrpms_last_error()
    for opt, (wording, _, refused) in OPTIONS.items():
        for v in refused:
            assert f(c, opt, v) == _lib.VRPMS_EINVAL, (opt, v)
            msg = lib.vrpms_last_error()
            assert b"vrpms_set_option" in msg and wording in msg, (opt, v, msg)
    assert fake.raw == bytes(1 << 16)


@pytest.mark.gpu
def test_set_option_accepts_its_values_and_a_refusal_leaves_no_trace(ctx):
    import numpy as np
    import torch
    from oracle import spec
    from vrpms_amd import _lib, synth
    from vrpms_amd.core import CVRP
    lib = ctx.lib
    static, td = synth.cvrp(30, 3, seed=1), synth.td_cvrp(20, 3, seed=3)

    def results():
        out = []
        for inst in (static, td):       # path 0 (eval_cvrp_rows2) and eval_staged
            ctx.set_instance(CVRP, inst.durations, inst.demand, inst.capacities, inst.start_times)
            P = synth.random_perms(700, inst.n, seed=2, ld=32)
            keys = ctx.eval(torch.from_numpy(P).to(ctx.dev), n=inst.n)
            k = keys.cpu().numpy().view(np.uint64)
            want = spec.eval_cvrp_batch(inst.durations, P[:, :inst.n], inst.demand,
                                        inst.capacities, inst.start_times)[0]
            assert (k == want.astype(np.uint64)).all()
            out.append(k)
        rng = np.random.default_rng(3)
        mats = rng.integers(3, 321, size=(5, 7, 7))
        mats[:, np.arange(7), np.arange(7)] = 0
        tours, keys = ctx.tsp_batch_dp(torch.tensor(mats, dtype=torch.int32, device=ctx.dev))
        return out + [tours.cpu().numpy(), keys.cpu().numpy()]

    before = results()
    for opt, (wording, accepted, refused) in OPTIONS.items():
        try:
            for v in accepted:
                assert lib.vrpms_set_option(ctx.handle, opt, v) == _lib.VRPMS_OK, (opt, v)
        finally:
            assert lib.vrpms_set_option(ctx.handle, opt, OPTION_DEFAULT.get(opt, 0)) == _lib.VRPMS_OK
        for v in refused:
            assert lib.vrpms_set_option(ctx.handle, opt, v) == _lib.VRPMS_EINVAL, (opt, v)
            assert wording in lib.vrpms_last_error()
    assert lib.vrpms_set_option(ctx.handle, 14, 1) == _lib.VRPMS_EINVAL
    for a, b in zip(before, results()):
        assert (a == b).all()


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vrpms_amd.core import Context
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Context(0)
