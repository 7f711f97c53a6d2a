"""Diagnostic: did a change touch device code?  Compares two directories of gfx950 assembly listings kernel by kernel.  Pure text, no GPU.

Make the listings once per tree, one per source of csrc/Makefile's SRCS:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S X.hip -o DIR/X.s
then   python tests/diag/isa_diff.py OLD_DIR NEW_DIR [--rename OLD_SUBSTRING=NEW_SUBSTRING ...]

A kernel is the text from its `NAME:` label through its last `s_endpgm` plus its `.amdhsa_kernel NAME` ... `.end_amdhsa_kernel` descriptor
(registers, LDS, scratch, kernarg size).  Local labels carry the function's index within the file (.LBB7_3), which moves when a kernel
before it comes or goes, so the index is dropped before comparing, and runs of blanks count as one (comments are aligned to a column).  Prints `same` / `differs` per file and kernel, the kernels only one
side has, and a summary line; exit status 1 when anything differs or is one-sided.  --rename pairs a kernel that moved or changed its
name: the substring is replaced in the OLD side's names and text (e.g. --rename 9k_voc_out=...)."""
import os
import re
import sys

LOCAL = re.compile(r"(BB|LJTI|Lfunc_begin|Lfunc_end|Ltmp|LCPI)\d+")      # also "Header=BB7_6" inside comments


def kernels(path, renames):
	text = open(path).read()
	for old, new in renames:
		text = text.replace(old, new)
	lines = text.split("\n")
	out = {}
	for i, line in enumerate(lines):
		m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
		if not m:
			continue
		name = m.group(1)
		start = next((j for j in range(i, -1, -1) if lines[j].startswith(name + ":")), None)
		end = next((j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel"), None)
		if start is None or end is None:
			raise SystemExit(f"{path}: kernel {name} has no label or no end of descriptor")
		last = max(j for j in range(start, i) if lines[j].split(";")[0].strip() == "s_endpgm")
		out[name] = [" ".join(LOCAL.sub(r"\1", l).split()) for l in lines[start:last + 1] + lines[i:end + 1]]
	return out


def main(argv):
	renames = []
	while "--rename" in argv:
		k = argv.index("--rename")
		renames.append(tuple(argv[k + 1].split("=", 1)))
		del argv[k:k + 2]
	if len(argv) != 3:
		raise SystemExit(__doc__)
	a_dir, b_dir = argv[1], argv[2]
	files = lambda d: {f for f in os.listdir(d) if f.endswith(".s")}
	same = differs = only = 0
	for f in sorted(files(a_dir) | files(b_dir)):
		a = kernels(os.path.join(a_dir, f), renames) if f in files(a_dir) else {}
		b = kernels(os.path.join(b_dir, f), []) if f in files(b_dir) else {}
		for name in sorted(set(a) | set(b)):
			if name not in b or name not in a:
				print(f"{f}: {name}: only in {a_dir if name in a else b_dir}")
				only += 1
			elif a[name] == b[name]:
				print(f"{f}: {name}: same")
				same += 1
			else:
				first = next((k for k, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
				print(f"{f}: {name}: differs (first at line {first} of the kernel, {len(a[name])} / {len(b[name])} lines)")
				differs += 1
	print(f"summary: {same} same, {differs} differ, {only} on one side only")
	return 1 if differs or only else 0


if __name__ == "__main__":
	sys.exit(main(list(sys.argv)))
