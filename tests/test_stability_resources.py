"""The stability kernels' resources in the code object (no GPU; scripts/kernel_resources.py, as
tests/test_kernel_resources.py reads it): every instantiation of 1-4 planets, planar and inclined, is there, none
has scratch or LDS beyond the count's partial sums, and a wave of the one-wave blocks fits its registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "rvel-mcmc_amd", "rvmcmc", "librvmcmc.so")


@pytest.fixture(scope="module")
def res():
    assert os.path.exists(LIB), "librvmcmc.so not built"
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not available")
    ks = KR.kernels(LIB)
    names = KR.demangle([k["name"] for k in ks])
    return {n.split("(")[0].replace("void ", ""): k for n, k in zip(names, ks)}


@pytest.mark.parametrize("kernel", ["stability_init_kernel", "stability_advance_kernel"])
@pytest.mark.parametrize("np_", [1, 2, 3, 4])
@pytest.mark.parametrize("d3", ["false", "true"])
def test_instantiation_exists_without_scratch(res, kernel, np_, d3):
    name = f"rvm::{kernel}<{np_}, {d3}>"
    assert name in res, [n for n in sorted(res) if "stability" in n]
    k = res[name]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["max_wg"] == 64, k  # one wave per block
    assert 0 < k["vgpr"] <= 512, k


def test_count_kernel(res):
    k = res["rvm::stability_count_kernel"]
    assert k["scratch"] == 0, k
