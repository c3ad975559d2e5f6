#!/bin/bash
# Whole device disassembly of every stage object of two builds, compared:  tools/stage_isa_compare.sh <other lib obj dir> [this lib obj dir]
# (tools/kernel_isa.sh prints one kernel; this hashes all of an object's device code, comments stripped, and says where two builds differ)
other=$(readlink -f $1); mine=$(readlink -f ${2:-$(dirname $0)/../slideo_amd/lib/obj})
tmp=$(mktemp -d)
dis() {  # <obj> <out>
    /opt/rocm/lib/llvm/bin/llvm-objcopy --dump-section .hip_fatbin=$tmp/fat.bin $1 2>/dev/null || { : > $2; return; }
    python3 -c "
d=open('$tmp/fat.bin','rb').read(); i=d.find(b'\x7fELF'); open('$tmp/co.elf','wb').write(d[i:])"
    /opt/rocm/lib/llvm/bin/llvm-objdump -d --mcpu=gfx950 $tmp/co.elf 2>/dev/null | sed 's/\/\/.*//' | grep -v "file format" > $2
}
rc=0
for st in stage_orb stage_knn stage_verify stage_sift stage_page_set stage_gate capi_runtime; do
    dis $other/$st.o $tmp/a.s; dis $mine/$st.o $tmp/b.s
    ha=$(md5sum < $tmp/a.s | cut -c1-32); hb=$(md5sum < $tmp/b.s | cut -c1-32)
    n=$(grep -c '^[0-9a-f]* <' $tmp/b.s)
    if [ "$ha" = "$hb" ]; then echo "$st: identical  $n symbols  $(wc -l < $tmp/b.s) lines  md5 $hb"
    else echo "$st: DIFFERS  other $ha  this $hb"; rc=1; fi
done
rm -rf $tmp
exit $rc
