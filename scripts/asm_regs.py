"""Register / spill summary of every kernel in build/asm (make -C open_l2o_amd/csrc asm: one .s per translation unit, the
kernels of csrc/l2o_ilp_kernels.h under max-ilp like the library's; or scripts/so_regs.py on the built library).
   python scripts/asm_regs.py [file.s ...] [--spills]"""
import glob, re, sys
args = [a for a in sys.argv[1:] if not a.startswith('--')] or sorted(glob.glob('build/asm/*.s'))
only_spills = '--spills' in sys.argv
for path in args:
    for b in open(path).read().split('  - .agpr_count:')[1:]:
        name = re.search(r'\.name:\s+(\S+)', b).group(1)
        ag = int(b.split('\n')[0])
        vg = int(re.search(r'\.vgpr_count:\s+(\d+)', b).group(1))
        sp = int(re.search(r'\.vgpr_spill_count:\s+(\d+)', b).group(1))
        sc = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1))
        if (sp or sc) if only_spills else True:
            print(f"{name[:80]:80s} agpr {ag:3d} total {vg:3d} spill {sp:3d} scratch {sc}")
