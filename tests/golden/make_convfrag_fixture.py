"""Records tests/golden/convfrag_packed.npz: the A fragments svs_conv2d_mfma_pack, svs_deconv2d_mfma_pack and
svs_conv3d_gemm_pack write for the cases of tests/wfrag_oracle.py (PACKED_CASES), as raw int16.  Run once on an MI355X at the
commit whose packers are the reference (the one before csrc/svs_conv_frag.h: each of the three had a kernel of its own):

    python tests/golden/make_convfrag_fixture.py [--svs <path to that commit's s-volsdf_amd>] [--out <file>]

tests/test_gpu_costvol.py::test_device_packers_match_the_torch_layouts compares today's library with it bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--svs", default=os.path.join(ROOT, "s-volsdf_amd"))
    ap.add_argument("--out", default=os.path.join(HERE, "convfrag_packed.npz"))
    a = ap.parse_args()
    sys.path[:0] = [a.svs, os.path.join(ROOT, "tests")]
    import wfrag_oracle as wo
    from svs_hip import costvol
    pack = {"conv2d": lambda w, _: costvol.conv2d_mfma_frag(w), "deconv2d": lambda w, _: costvol.deconv2d_mfma_frag(w),
            "gemm": costvol.gemm_weight_fragments}
    out = {}
    for key, (kind, _, arg) in wo.PACKED_CASES.items():
        w = wo.packed_case_weight(key).cuda()
        frag = pack[kind](w, arg)
        torch.cuda.synchronize()
        out[key] = frag.view(torch.int16).cpu().numpy().reshape(-1)
        print(key, out[key].size * 2, "bytes")
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes; packers of", os.path.abspath(a.svs))


if __name__ == "__main__":
    main()
