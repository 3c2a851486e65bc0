"""Register / scratch / occupancy report of every kernel in jb_api.hip (compiler remarks; no GPU needed), compiled with the flags the
library ships with (tools/asm_listing.py).

    python tools/kernel_resources.py [extra hipcc flags]"""
import re
import subprocess
import sys
import tempfile

import asm_listing


def rows(remarks):
    """{short kernel name: ["VGPRs 256", ...]} from the text of -Rpass-analysis=kernel-resource-usage"""
    name, out = None, {}
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = asm_listing.short_name(m.group(1))
            out[name] = []
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill): (\S+)", line)
        if m and name:
            out[name].append("%s %s" % (m.group(1).split(" ")[0], m.group(2)))
    return out


if __name__ == "__main__":
    with tempfile.NamedTemporaryFile(suffix=".o") as obj:
        cmd = asm_listing.compile_command(["-c"], obj.name, ["-Rpass-analysis=kernel-resource-usage"] + sys.argv[1:])
        table = rows(subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout)
    for k in sorted(table):
        print("%-60s %s" % (k[:60], " | ".join(table[k])))
