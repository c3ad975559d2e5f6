#!/bin/bash
# Whole device disassembly of every stage object of two builds, compared:  tools/stage_isa_compare.sh <other lib obj dir> [this lib obj dir]
# (tools/kernel_isa.sh prints one kernel; this hashes all of an object's device code, comments stripped, and says where two builds differ:
# an object that differs as a whole is compared kernel by kernel)
other=$(readlink -f $1); mine=$(readlink -f ${2:-$(dirname $0)/../slideo_amd/lib/obj})
tmp=$(mktemp -d)
dis() {  # <obj> <out>
    /opt/rocm/lib/llvm/bin/llvm-objcopy --dump-section .hip_fatbin=$tmp/fat.bin $1 2>/dev/null || { : > $2; return; }
    python3 -c "
d=open('$tmp/fat.bin','rb').read(); i=d.find(b'\x7fELF'); open('$tmp/co.elf','wb').write(d[i:])"
    /opt/rocm/lib/llvm/bin/llvm-objdump -d --mcpu=gfx950 $tmp/co.elf 2>/dev/null | sed 's/\/\/.*//' | grep -v "file format" > $2
}
rc=0
for st in stage_orb stage_knn stage_verify stage_sift stage_page_set stage_gate stage_direct stage_ssd_table stage_activity stage_gate_anchor stage_content capi_runtime; do
    dis $other/$st.o $tmp/a.s; dis $mine/$st.o $tmp/b.s
    ha=$(md5sum < $tmp/a.s | cut -c1-32); hb=$(md5sum < $tmp/b.s | cut -c1-32)
    n=$(grep -c '^[0-9a-f]* <' $tmp/b.s)
    if [ "$ha" = "$hb" ]; then echo "$st: identical  $n symbols  $(wc -l < $tmp/b.s) lines  md5 $hb"
    else
        # per kernel: the text of each symbol without its address (a unit that gained kernels differs as a whole; the kernels both
        # builds have must still be the same code)
        python3 - $tmp/a.s $tmp/b.s > $tmp/per.txt <<'PY'
import hashlib, re, subprocess, sys
def names(path):                                # every symbol of a listing, demangled in one c++filt run
    found = [m.group(1) for m in (re.match(r'^[0-9a-f]+ <(.+)>:', l) for l in open(path)) if m]
    out = subprocess.run(['c++filt'], input='\n'.join(found), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(found, out))
def key(d):                                     # kernel name and template arguments without the trailing parameter list, so that a
    if not d.endswith(')'): return d            # kernel whose argument record was renamed pairs up; nothing else of the name goes
    depth = 0
    for i in range(len(d) - 1, -1, -1):
        depth += (d[i] == ')') - (d[i] == '(')
        if depth == 0: return re.sub(r'^void ', '', d[:i])
    return d
def syms(path):
    out, cur, dem = {}, None, names(path)
    for line in open(path):
        m = re.match(r'^[0-9a-f]+ <(.+)>:', line)
        if m:
            cur = key(dem[m.group(1)])
            if cur in out: cur = m.group(1)     # (two symbols of one key, overloads: keep both, under their mangled names)
            out[cur] = []
        elif cur is not None and line.strip():
            out[cur].append(re.sub(r'\s+', ' ', line.strip()))
    for v in out.values():                      # (the alignment padding behind a kernel depends on what follows it)
        while v and v[-1] in ('s_nop 0', 's_code_end', '...'): v.pop()
    return {k: hashlib.md5('\n'.join(v).encode()).hexdigest() for k, v in out.items()}
a, b = syms(sys.argv[1]), syms(sys.argv[2])
bad = 0
for k in sorted(set(a) | set(b)):
    if k not in a: print('    only this   %s' % k)
    elif k not in b: print('    only other  %s' % k); bad = 1
    elif a[k] == b[k]: print('    identical   %s  md5 %s' % (k, a[k]))
    else: print('    DIFFERS     %s' % k); bad = 1
sys.exit(bad)
PY
        if [ $? = 0 ]; then echo "$st: every kernel of the other build identical, new kernels added  other $ha  this $hb"
        else echo "$st: DIFFERS  other $ha  this $hb"; rc=1; fi
        cat $tmp/per.txt
    fi
done
rm -rf $tmp
exit $rc
