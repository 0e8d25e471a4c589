"""Compare the gfx950 device code of two builds of libifcbk.so, kernel by kernel (no GPU needed).

  python scripts/isa_compare.py OLD/libifcbk.so NEW/libifcbk.so

For every kernel present in both builds: the mnemonic sequence of its disassembly must be the same, and so must its VGPR / AGPR /
SGPR counts, LDS size and scratch size from the code-object metadata.  Operands may differ only in immediates (a removed field of
an argument block shifts kernarg offsets).  Prints the kernels only one build has and every difference; exit status 1 on a mismatch
of a common kernel.  Uses llvm-objdump / llvm-readelf of the ROCm install (ROCM_PATH, default /opt/rocm).
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
META = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def code_objects(so):
    """the gfx950 ELF images of every offload bundle in the library"""
    blob = open(so, 'rb').read()
    out, i = [], blob.find(MAGIC)
    while i >= 0:
        n = struct.unpack_from('<Q', blob, i + 24)[0]
        off = i + 32
        for _ in range(n):
            o, size, tlen = struct.unpack_from('<QQQ', blob, off)
            triple = blob[off + 24:off + 24 + tlen].decode()
            off += 24 + tlen
            if 'gfx950' in triple and size:
                out.append(blob[i + o:i + o + size])
        i = blob.find(MAGIC, i + 1)
    return out


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), stdout=subprocess.PIPE, text=True, check=True).stdout


def kernels(so):
    """kernel symbol -> (instructions [(mnemonic, operands with immediates blanked, operands)], metadata {key: value})"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, co in enumerate(code_objects(so)):
            path = os.path.join(tmp, 'co%d.elf' % k)
            with open(path, 'wb') as fh:
                fh.write(co)
            meta = _kernel_meta(_run('llvm-readelf', '--notes', path))
            name, insts = None, None
            for ln in _run('llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', path).splitlines():
                m = re.match(r'^<(.+)>:$', ln)
                if m:
                    name = m.group(1)
                    insts = [] if name in meta else None
                    if insts is not None:
                        res[name] = (insts, meta[name])
                    continue
                if insts is None or not ln.strip() or ln.strip().startswith(';'):
                    continue
                body = ln.split('//')[0].strip()
                if not body:
                    continue
                mn, _, ops = body.partition(' ')
                ops = ops.strip()
                insts.append((mn, re.sub(r'(?<![\w.])-?(0x[0-9a-fA-F]+|\d+(\.\d+)?)\b', '#', ops), ops))
    return res


def _kernel_meta(notes):
    """{kernel symbol: {metadata key: value}} from the AMDGPU metadata note (one YAML list item per kernel)"""
    out = {}
    block = []

    def flush():
        d = {}
        for s in block:
            for key in META + ('.symbol',):
                if s.startswith(key + ':'):
                    d.setdefault(key, s.split(':', 1)[1].strip())
        if '.symbol' in d:
            out[d.pop('.symbol')[:-3]] = d
    for ln in notes.splitlines():
        s = ln.strip()
        if s.startswith('- .'):                      # a list item: a kernel when at the top indent, else an argument
            if re.match(r'^  - \.', ln):
                flush()
                block = []
            s = s[2:]
        block.append(s)
    flush()
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    for name in sorted(set(a) - set(b)):
        print('only in %s: %s' % (old, name))
    for name in sorted(set(b) - set(a)):
        print('only in %s: %s' % (new, name))
    nimm = 0
    for name in sorted(set(a) & set(b)):
        (ia, ma), (ib, mb) = a[name], b[name]
        if [x[0] for x in ia] != [x[0] for x in ib]:
            print('MNEMONICS DIFFER: %s (%d vs %d instructions)' % (name, len(ia), len(ib)))
            bad += 1
            continue
        if ma != mb:
            print('METADATA DIFFERS: %s %s vs %s' % (name, ma, mb))
            bad += 1
        ops = [(x, y) for x, y in zip(ia, ib) if x[2] != y[2]]
        if any(x[1] != y[1] for x, y in ops):
            print('OPERANDS DIFFER beyond immediates: %s, e.g. %s' % (name, next((x[2], y[2]) for x, y in ops if x[1] != y[1])))
            bad += 1
        nimm += bool(ops)
    print('%d kernels in both builds, %d only in the old, %d only in the new; %d differ in immediates only; %d mismatches'
          % (len(set(a) & set(b)), len(set(a) - set(b)), len(set(b) - set(a)), nimm, bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
