"""Register and scratch use of the dense GEMM kernels (csrc/gemm.hip), read from the gfx950 code object inside the built csrc/build/gemm.o -- no GPU needed.

The hand-ordered k-loops issue their LDS fragment reads and DMA pieces from inline asm, invisible to the compiler's wait-count pass: they are correct only
as long as the register allocator puts no copy or spill between such a read and the hand-written `s_waitcnt lgkmcnt(0)` that ends its step.  A spill or
scratch slot that appears in a kernel is therefore something to look at, not a detail: every GEMM kernel reports zero VGPR spills, zero SGPR spills and
zero private segment bytes, except those on the list below, each held to its present values as upper bounds and with the reason it is harmless."""
import os
import re
import shutil
import subprocess

import pytest

from tortoise_tts_amd import _lib

LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
GEMM_O = os.path.join(_lib.HERE, "csrc", "build", "gemm.o")

_HAND_ORDERED_SCRATCH = ("the k = 3 tap table va3[3][2] (the six per-lane A staging offsets, 24 B) lives in scratch: stored once in the prologue, two "
						 "scratch_load_dword per tap change; ISA read: no scratch access between a pipe_read16 and its s_waitcnt lgkmcnt(0), and the extra "
						 "vector-memory loads only make the counted vmcnt waits stricter (in-order retire) -- cost, not correctness")
_COMPILER_ORDERED_SPILL = ("compiler-ordered k-loop (no asm fragment reads at 256 x 128 for this role): the wait-count pass sees its own spill traffic; "
						   "most spill code lies in the residual / statistics epilogue")
# kernel -> (vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size) upper bounds, reason
ALLOW = {
	"k_gemm<bf16,128,128,2,4,3,GR_CONV3_RES>": ((0, 0, 32), "hand-ordered PIPE stream, 64 x 32 wave block: " + _HAND_ORDERED_SCRATCH),
	"k_gemm<f16,128,128,2,4,3,GR_CONV3_RES>": ((0, 0, 32), "hand-ordered PIPE stream, 64 x 32 wave block: " + _HAND_ORDERED_SCRATCH),
	"k_gemm<bf16,256,128,4,2,3,GR_CONV3_RES>": ((15, 0, 112), _COMPILER_ORDERED_SPILL),
	"k_gemm<f16,256,128,4,2,3,GR_CONV3_RES>": ((15, 0, 112), _COMPILER_ORDERED_SPILL),
	"k_gemm<bf16,256,128,4,2,3,GR_PROJ_RES>": ((24, 0, 100), _COMPILER_ORDERED_SPILL),
	"k_gemm<f16,256,128,4,2,3,GR_PROJ_RES>": ((24, 0, 100), _COMPILER_ORDERED_SPILL),
	"k_gemm<f8,256,128,4,2,3,GR_CONV3_RES>": ((17, 0, 128), "fp8 operands never run the hand-ordered loops: " + _COMPILER_ORDERED_SPILL),
	"k_gemm<f8,256,128,4,2,3,GR_PROJ_RES>": ((17, 0, 68), "fp8 operands never run the hand-ordered loops: " + _COMPILER_ORDERED_SPILL),
}
ROLES = {0: "GR_NONE", 1: "GR_IN1x1", 2: "GR_CONV3_RES", 3: "GR_QKV", 4: "GR_PROJ_RES"}
TYPES = {"f": "f32", "DF16b": "bf16", "DF16_": "f16", "NS_2f8E": "f8"}


def kernel_name(sym):
	"""_ZN3ttk6k_gemmIDF16bLi128ELi128ELi2ELi4ELi3ELi2ELb0EEEvNS_10GemmParamsE -> k_gemm<bf16,128,128,2,4,3,GR_CONV3_RES> (LONGK appended when set)"""
	m = re.fullmatch(r"_ZN3ttk\d+(k_gemm(?:_mixed)?)I(f|DF16b|DF16_|NS_2f8E)((?:L[ib]-?\d+E)*)EEvNS_10GemmParamsE", sym)
	assert m, f"unexpected GEMM kernel symbol {sym}"
	args = [int(x) for x in re.findall(r"L[ib](-?\d+)E", m.group(3))]
	t = TYPES[m.group(2)]
	if m.group(1) == "k_gemm_mixed":
		return f"k_gemm_mixed<{t},{ROLES[args[0]]}>"
	bm, bn, nwm, nwn, ns, role, longk = args
	return f"k_gemm<{t},{bm},{bn},{nwm},{nwn},{ns},{ROLES[role]}{',LONGK' if longk else ''}>"


def gemm_code_object(tmp_path, tools=TOOLS, obj=GEMM_O):
	"""(tool paths, path of the gfx950 code object taken out of csrc/build/gemm.o, or out of another object file of the build)"""
	paths = {t: shutil.which(t, path=LLVM_BIN) for t in tools}
	if not all(paths.values()):
		pytest.skip(f"ROCm LLVM tools missing under {LLVM_BIN}: {[t for t, p in paths.items() if not p]}")
	_lib.build()
	stem = os.path.splitext(os.path.basename(obj))[0]
	fatbin, co = str(tmp_path / f"{stem}.fatbin"), str(tmp_path / f"{stem}.gfx950.co")
	subprocess.run([paths["llvm-objcopy"], f"--dump-section=.hip_fatbin={fatbin}", obj, str(tmp_path / "discard.o")], check=True, capture_output=True)
	subprocess.run([paths["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fatbin}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
					f"--output={co}"], check=True, capture_output=True)
	return paths, co


def kernel_metadata(tmp_path, keys, symbol, obj=GEMM_O):
	"""{kernel symbol: tuple of the integer fields `keys`} from the code-object notes of `obj`, for the kernels whose symbol matches the pattern `symbol`"""
	paths, co = gemm_code_object(tmp_path, obj=obj)
	notes = subprocess.run([paths["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
	out = {}
	for block in re.split(r"\n\s*- \.(?=agpr_count|args)", notes):
		name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
		if not name or not re.match(symbol, name.group(1)):
			continue

		def field(key):
			v = re.search(rf"^\s*\.{key}:\s+(\d+)", block, re.M)
			assert v, f"{name.group(1)}: no .{key} in the code-object metadata"
			return int(v.group(1))
		out[name.group(1)] = tuple(field(k) for k in keys)
	return out


def gemm_kernel_resources(tmp_path):
	res = kernel_metadata(tmp_path, ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"), r"_ZN3ttk\d+k_gemm")
	return {kernel_name(sym): v for sym, v in res.items()}


def test_gemm_kernels_have_no_spills_or_scratch_beyond_the_allowlist(tmp_path):
	res = gemm_kernel_resources(tmp_path)
	assert len(res) >= 80, f"only {len(res)} GEMM kernels found in the code object"
	assert any(k.startswith("k_gemm_mixed<") for k in res) and "k_gemm<bf16,256,128,4,2,3,GR_NONE,LONGK>" in res
	bad = []
	for k, v in sorted(res.items()):
		bound = ALLOW.get(k, ((0, 0, 0), None))[0]
		if any(x > b for x, b in zip(v, bound)):
			bad.append(f"{k}: (vgpr spill, sgpr spill, scratch B) = {v} > {bound}")
	for k, (bound, why) in ALLOW.items():
		print(f"allowed {k} <= {bound}: {why}")
	missing = sorted(set(ALLOW) - set(res))
	assert not missing, f"allowlisted kernels no longer built (drop them from ALLOW): {missing}"
	assert not bad, "GEMM kernels spill or use scratch beyond the allowlist:\n" + "\n".join(bad)


def test_kernel_name_reading():
	assert kernel_name("_ZN3ttk6k_gemmIDF16bLi128ELi128ELi2ELi4ELi3ELi2ELb0EEEvNS_10GemmParamsE") == "k_gemm<bf16,128,128,2,4,3,GR_CONV3_RES>"
	assert kernel_name("_ZN3ttk6k_gemmIDF16_Li256ELi128ELi4ELi2ELi3ELi0ELb1EEEvNS_10GemmParamsE") == "k_gemm<f16,256,128,4,2,3,GR_NONE,LONGK>"
	assert kernel_name("_ZN3ttk12k_gemm_mixedINS_2f8ELi4EEEvNS_10GemmParamsE") == "k_gemm_mixed<f8,GR_PROJ_RES>"
	assert kernel_name("_ZN3ttk6k_gemmIfLi64ELi64ELi2ELi2ELi3ELi0ELb0EEEvNS_10GemmParamsE") == "k_gemm<f32,64,64,2,2,3,GR_NONE>"


def test_gemm_kernels_touch_m0_only_by_scalar_moves(tmp_path):
	"""The hand-ordered k-loops write M0 from inline asm without declaring it (csrc/gemm_prims.h, "M0 INVARIANT"): they save it in front of the loop, restore
	it behind, and rely on the compiler using M0 nowhere in a GEMM kernel.  Held here on the disassembled code object: every instruction of a k_gemm* kernel
	that names m0 is `s_mov_b32 m0, sN` (an LDS-DMA piece's base, or the restore) or `s_mov_b32 sN, m0` (the save)."""
	paths, co = gemm_code_object(tmp_path, TOOLS + ("llvm-objdump",))
	text = subprocess.run([paths["llvm-objdump"], "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
	ok = re.compile(r"s_mov_b32 (m0, s\d+|s\d+, m0)$")
	kernel, seen, writes, reads, bad = None, set(), 0, 0, []
	for line in text.split("\n"):
		label = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
		if label:
			kernel = label.group(1) if re.match(r"_ZN3ttk\d+k_gemm", label.group(1)) else None
			seen.add(kernel)
			continue
		ins = line.split("//")[0].strip()
		if kernel and re.search(r"\bm0\b", ins):
			if not ok.search(ins):
				bad.append(f"{kernel_name(kernel)}: {ins}")
			writes += " m0, " in ins
			reads += ins.endswith(", m0")
	seen.discard(None)
	print(f"{len(seen)} GEMM kernels: {writes} moves into m0, {reads} moves out of m0")
	assert len(seen) >= 80 and writes > 0 and reads > 0, f"{len(seen)} GEMM kernels, {writes} / {reads} m0 moves found in the disassembly"
	assert not bad, "GEMM kernels use m0 other than by s_mov_b32 to / from an SGPR:\n" + "\n".join(bad[:40])
