"""Which kernels of two built libl2o_hip.so differ in their ISA?  (A change that claims to touch ONE kernel family shows it here.)
   python scripts/so_isa_diff.py old.so new.so [name-substring]
Unbundles the gfx950 code objects (like scripts/so_regs.py), disassembles them with llvm-objdump and compares the
instruction text of every kernel symbol -- addresses and encodings stripped, so a kernel that merely moved compares equal.
Prints one line per kernel that differs (instructions old -> new, lines changed) and the count of identical ones."""
import difflib, re, struct, subprocess, sys, tempfile

OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def kernels(lib):
    data = open(lib, 'rb').read()
    out, start = {}, 0
    while True:
        i = data.find(MAGIC, start)
        if i < 0:
            return out
        start = i + len(MAGIC)
        n, = struct.unpack_from('<Q', data, i + 24)
        pos = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', data, pos)
            triple = data[pos + 24:pos + 24 + tl].decode()
            pos += 24 + tl
            if 'gfx950' not in triple:
                continue
            with tempfile.NamedTemporaryFile(suffix='.co') as f:
                f.write(data[i + off:i + off + size]); f.flush()
                txt = subprocess.run([OBJDUMP, '-d', '--no-show-raw-insn', f.name], capture_output=True, text=True).stdout
            name = None
            for line in txt.split('\n'):
                m = re.match(r'^[0-9a-f]+ <(\S+)>:', line)
                if m:
                    name = m.group(1)
                    out[name] = []
                elif name and line.strip():
                    out[name].append(re.sub(r'\s*//.*$', '', line).strip())


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else ''
    same = 0
    for name in sorted(set(a) | set(b)):
        if pat not in name:
            continue
        if name not in a or name not in b:
            print('%-9s %s' % ('only old' if name in a else 'only new', name))
        elif a[name] == b[name]:
            same += 1
        else:
            changed = sum(1 for l in difflib.unified_diff(a[name], b[name], lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---'))
            print('DIFFERS   %-110s %5d -> %5d instructions, %d diff lines' % (name[:110], len(a[name]), len(b[name]), changed))
    print('%d kernels identical' % same)


if __name__ == '__main__':
    main()
