"""Turns the CSV files of `rocprofv3 --hip-trace --kernel-trace --output-format csv` into the two lists compared in bench.md:
   <name>.hip_calls.txt  the HIP calls that go to a stream, in start order
   <name>.kernels.txt    every kernel dispatch in dispatch order, with grid, block and LDS
Usage: lists.py <directory with t_hip_api_trace.csv and t_kernel_trace.csv> <output prefix>"""
import csv
import os
import sys

STREAM_SIDE = {"hipLaunchKernel", "hipMemcpyAsync", "hipMemsetAsync", "hipMemcpy", "hipMemset", "hipEventRecord", "hipStreamWaitEvent", "hipStreamSynchronize"}


def main(src, prefix):
    with open(os.path.join(src, "t_hip_api_trace.csv")) as f:
        calls = sorted((int(r["Start_Timestamp"]), r["Function"]) for r in csv.DictReader(f) if r["Function"] in STREAM_SIDE)
    with open(prefix + ".hip_calls.txt", "w") as f:
        f.writelines(name + "\n" for _, name in calls)
    with open(os.path.join(src, "t_kernel_trace.csv")) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    with open(prefix + ".kernels.txt", "w") as f:
        for r in rows:
            # (the descriptors GsRun / GsCombineCol left the anonymous namespace: the kernels' names are compared without it)
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "")
            f.write(f"{name} grid=({r['Grid_Size_X']},{r['Grid_Size_Y']},{r['Grid_Size_Z']}) "
                    f"block=({r['Workgroup_Size_X']},{r['Workgroup_Size_Y']},{r['Workgroup_Size_Z']}) lds={r['LDS_Block_Size']}\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
