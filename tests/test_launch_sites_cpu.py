"""Every kernel launch under csrc/ goes through launch_checked (csrc/launch.hpp) or launch_checked_ev (csrc/aux_stream.hpp): a text scan."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnn_rul_benchmarking_amd", "csrc")
HELPERS = {"launch.hpp", "aux_stream.hpp"}            # the only files that may launch a kernel or read the runtime's last error
RAW = re.compile(r"hipLaunchKernelGGL|hipExtLaunchKernelGGL|<<<|hipGetLastError")


def test_launches_go_through_launch_checked():
    names = sorted(os.listdir(CSRC))
    assert HELPERS <= set(names)
    bad = []
    for name in names:
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                if "RULGNN_LAUNCH_OK" in line or (name not in HELPERS and RAW.search(line)):
                    bad.append(f"csrc/{name}:{no}: {line.strip()}")
    assert not bad, "launch through launch_checked (csrc/launch.hpp) and propagate its status with RULGNN_TRY:\n" + "\n".join(bad)
