"""Per-symbol comparison of two device assembly files (hipcc --cuda-device-only -S of one translation unit -- or the .s files of
make -C open_l2o_amd/csrc asm, concatenated -- before and after a change that must not touch device code): the same functions, each with the same instructions, the same .amdhsa_ descriptor
and the same metadata entry.  Function ORDER may differ, so the numbers in local labels are normalised.
  python scripts/asm_kernel_diff.py before.s after.s"""
import re, sys

def symbols(path):
    s = re.sub(r'\b(L?BB|Ltmp|Lfunc_begin|Lfunc_end|LJTI|LCPI)\d+', r'\1', open(path).read())   # (.LBB12_3 and the BB12_3 of comments)
    s = re.sub(r'[ \t]+;', ' ;', s)                  # (comments are aligned behind the label, whose length changed)
    out = {}
    for m in re.finditer(r'^(\S+):\s+; @\1\n(.*?)^\.Lfunc_end:', s, re.M | re.S):
        out['code ' + m.group(1)] = m.group(2)
    for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel', s, re.M | re.S):
        out['desc ' + m.group(1)] = m.group(2)
    for b in s.split('  - .agpr_count:')[1:]:
        out['meta ' + re.search(r'\.name:\s+(\S+)', b).group(1)] = b.split('\namdhsa.target')[0].rstrip()   # (the last entry of a file has no newline)
    return out

a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
for k in sorted(set(a) ^ set(b)): print(('only before: ' if k in a else 'only after:  ') + k)
diff = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
for k in diff: print('differs:     ' + k)
n = lambda d, p: sum(k.startswith(p) for k in d)
print(f"before: {n(a, 'desc ')} kernels, {n(a, 'code ') - n(a, 'desc ')} other functions; after: {n(b, 'desc ')} kernels, "
      f"{n(b, 'code ') - n(b, 'desc ')} other functions; {len(diff)} differ, {len(set(a) ^ set(b))} unmatched")
sys.exit(1 if diff or set(a) ^ set(b) else 0)
