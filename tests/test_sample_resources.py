"""Spills, scratch and LDS of the token-step kernels (csrc/sample.hip, sample_ext.hip, beam.hip), read from the code-object notes of the built objects -- no
GPU needed.

The three files build their kernels from one set of forced-inline stages (csrc/sample_stages.h, sample_prims.h) on a row of nine values per thread held in
registers, in 1024-thread blocks: 128 VGPRs is all such a block may hold, and k_sample_step_ext sits a few registers below that.  A stage edited for one
kernel is edited for all of them, so a spill or a scratch slot it causes elsewhere has to show up here: every kernel reports zero VGPR spills and zero
private segment bytes, and no more LDS than when the stages were folded out of the kernels (the values below).  Metadata only; no instruction is looked at."""
import os

import pytest

from test_gemm_resources import kernel_metadata
from tortoise_tts_amd import _lib

BUILD = os.path.join(_lib.HERE, "csrc", "build")
# object file -> {kernel symbol: LDS bytes (group_segment_fixed_size) upper bound}
KERNELS = {
	"sample.o": {"_ZN3ttk13k_sample_stepILb0EEEvNS_12SampleParamsE": 4376, "_ZN3ttk13k_sample_stepILb1EEEvNS_12SampleParamsE": 3352},
	"sample_ext.o": {"_ZN3ttk17k_sample_step_extENS_15SampleExtParamsE": 24080},
	"beam.o": {"_ZN3ttk13k_beam_scoresENS_10BeamParamsE": 4304, "_ZN3ttk13k_beam_selectENS_10BeamParamsE": 1992},
}


@pytest.mark.parametrize("obj", list(KERNELS))
def test_token_step_kernels_have_no_spills_no_scratch_and_no_more_lds(tmp_path, obj):
	res = kernel_metadata(tmp_path, ("vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"), r"_ZN3ttk\d+k_(sample_step|beam_s)",
						  obj=os.path.join(BUILD, obj))
	assert set(res) == set(KERNELS[obj]), f"{obj}: kernels found {sorted(res)}"
	for sym, lds_bound in KERNELS[obj].items():
		spill, scratch, lds = res[sym]
		print(f"{sym}: vgpr spill {spill}, scratch {scratch} B, LDS {lds} B (bound {lds_bound})")
		assert spill == 0, f"{sym}: {spill} VGPR spills"
		assert scratch == 0, f"{sym}: {scratch} B of scratch"
		assert lds <= lds_bound, f"{sym}: {lds} B of LDS, above {lds_bound}"
