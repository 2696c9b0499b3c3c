"""CPU check of the built gfx950 code objects (no GPU): the library holds exactly one
k_motions_clearance and one k_traj_chord_clearance, and both keep every value in registers --
no private-segment (scratch) memory and no spilled VGPRs -- by the compiler's metadata, read
as test_kernel_resources.py reads it.  Resource figures only."""
import os

import pytest

from eppamd import capi
from test_kernel_resources import LLVM, _kernel_metadata


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="ROCm LLVM tools absent")
def test_edge_clearance_kernels_do_not_spill():
    meta = _kernel_metadata(capi.LIB_PATH)
    for kernel in ("k_motions_clearance", "k_traj_chord_clearance"):
        found = {k: v for k, v in meta.items() if kernel in k}
        assert len(found) == 1, (kernel, sorted(found))
        (name, v), = found.items()
        print(name, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (name, v)
        assert v.get("vgpr_spill_count", 0) == 0, (name, v)
        assert 0 < v["vgpr_count"] <= 256, (name, v)
