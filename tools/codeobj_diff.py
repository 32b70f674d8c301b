#!/usr/bin/env python
"""Are the gfx950 kernels of two builds of librenet_hip.so the same machine code?  (No GPU needed.)

  python tools/codeobj_diff.py OLD/librenet_hip.so NEW/librenet_hip.so

Extracts every gfx950 code object from the libraries' .hip_fatbin sections, disassembles them (llvm-objdump) and reads the
kernel metadata (llvm-readelf --notes), then compares kernel by kernel, keyed by mangled name: the instruction text
(mnemonics, operands and encodings; addresses dropped) and .vgpr_count, .sgpr_count, .group_segment_fixed_size,
.private_segment_fixed_size, .max_flat_workgroup_size.  Prints the kernels that differ, the ones only one side has, and a
summary line; exit status 1 unless every kernel of OLD is in NEW unchanged and NEW adds none (expected removals are named
with --removed SUBSTRING, repeatable).
"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
META = ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size', '.max_flat_workgroup_size')


def code_objects(lib, tmp):
    """gfx950 ELF images inside lib's .hip_fatbin (one uncompressed bundle per translation unit)."""
    fat = os.path.join(tmp, 'fatbin')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', lib, fat])
    blob = open(fat, 'rb').read()
    out = []
    pos = blob.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from('<Q', blob, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if 'gfx950' in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + 1)
    if not out:
        raise SystemExit('%s: no gfx950 code object found (compressed bundles are not handled)' % lib)
    return out


def kernels(lib):
    """{mangled name: (instruction text, metadata dict)} over all code objects of lib."""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, img in enumerate(code_objects(lib, tmp)):
            co = os.path.join(tmp, 'co%d.elf' % i)
            open(co, 'wb').write(img)
            notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
            meta = {}
            for block in notes.split('  - .agpr_count')[1:]:
                name = re.search(r'^\s+\.name:\s+(\S+)', block, re.M).group(1)
                meta[name] = {k: re.search(r'^\s+%s:\s+(\S+)' % re.escape(k), block, re.M).group(1) for k in META}
            dis = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', co], text=True)
            cur = None
            for line in dis.split('\n'):
                m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
                if m:
                    cur = m.group(1)
                    if cur in meta:
                        assert cur not in res, 'kernel %s in two code objects' % cur
                        res[cur] = ([], meta[cur])
                    continue
                if cur in meta and line.strip() and line.strip() != '...':       # '...': zero padding up to the next symbol
                    # "insn operands   // 000000001234: ENCODING" -> drop the address, keep the encoding
                    res[cur][0].append(re.sub(r'//\s*[0-9A-Fa-f]+:', '//', line).strip())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--removed', action='append', default=[], help='substring of a kernel name that NEW is expected to lack')
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    same, differ, missing, expected = 0, [], [], []
    for name, (text, meta) in sorted(old.items()):
        if name not in new:
            (expected if any(s in name for s in a.removed) else missing).append(name)
        elif new[name][0] != text or new[name][1] != meta:
            differ.append(name)
        else:
            same += 1
    added = sorted(set(new) - set(old))
    for title, names in (('DIFFERENT', differ), ('MISSING', missing), ('ADDED', added), ('removed as expected', expected)):
        for n in names:
            print('%s: %s' % (title, n))
    print('kernels in old %d, in new %d: identical %d, different %d, missing %d, added %d, removed as expected %d'
          % (len(old), len(new), same, len(differ), len(missing), len(added), len(expected)))
    return 0 if not (differ or missing or added) else 1


if __name__ == '__main__':
    sys.exit(main())
