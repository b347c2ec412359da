#!/bin/bash
# Register / scratch / occupancy figures, code length and a digest of the instruction text of every kernel of a source file of
# rayn_amd/csrc/ as the product flags compile it (policy 0; default kernels.hip).
#   tools/kernel_resources.sh [kernels.hip] [extra hipcc flags]
# To compare two builds, run it on the same file at both commits and diff the outputs: a kernel whose line is the same has the same
# instructions.  The digest is over the kernel's assembly with comments, blank lines, the numbering of local labels and any line that
# names the per-build __hip_cuid_ symbol left out; it hashes and counts, nothing else.
here=$(cd "$(dirname "$0")/.." && pwd)
src=${1:-$here/rayn_amd/csrc/kernels.hip}; shift
asm=$(mktemp /tmp/kernel_resources.XXXXXX.s)
trap 'rm -f "$asm"' EXIT
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -mllvm -align-all-nofallthru-blocks=5 -fPIC \
  -I"$here/rayn_amd/csrc" -DRAYN_FMA_POLICY=0 -DRAYN_KNS=rayn_p0 "$@" -Rpass-analysis=kernel-resource-usage --cuda-device-only -S -o "$asm" "$src" 2>&1 | python3 -c "
import hashlib, re, subprocess, sys
cur = None; d = {}
for l in sys.stdin:
    m = re.search(r'Function Name: (\S+)', l)
    if m: cur = m.group(1); d[cur] = {}; continue
    m = re.search(r'remark:\s+(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)', l)
    if m and cur: d[cur][m.group(1).split(' [')[0]] = int(m.group(2))
# the assembly: a function runs from its label to its .Lfunc_end; '; codeLenInByte = N' follows in the function's trailer
cur = None; text = []
for l in open(sys.argv[1]):
    m = re.match(r'(\w+):', l)
    if m and m.group(1) in d: cur = m.group(1); text = []; continue
    m = re.search(r'; codeLenInByte = (\d+)', l)
    if m and cur: d[cur]['CodeLen'] = int(m.group(1)); cur = None; continue
    if cur is None or text is None: continue
    if l.startswith('.Lfunc_end'):
        d[cur]['Digest'] = hashlib.sha256('\n'.join(text).encode()).hexdigest()[:16]; text = None; continue
    l = re.sub(r'\.LBB\d+_', '.LBB_', l.split(';')[0]).strip()
    if l and '__hip_cuid_' not in l: text.append(l)
for k, v in d.items():
    name = subprocess.run(['c++filt', k], capture_output=True, text=True).stdout.strip()
    print(re.sub(r'\(.*', '', name.replace('(anonymous namespace)::', '')).replace('rayn_p0::', '').replace('void ', ''), v)
" "$asm"
