#!/usr/bin/env python3
"""Run ON THE GPU BOX: random SEQUENCES OF SCENE EDITS (tests/scene_edit_model.py: instance tables resent, moved, mirrored, re-pointed, grown
and shrunk; position, index, texcoord, colour and tangent streams rewritten; pt_skin_run; pt_accel_request_rebuild; a change of builder; refused
calls), 0-4 of them before each pt_build_accel, pt_trace, pt_lens_focus_at, pt_motion_snapshot, pt_debug_intersect or pt_debug_accel_read.  After
every one of those the checks of tests/test_gpu_scene_edits.py: the build / refit / nothing decision against the model of include/mipt.h, the
tree node by node and packet by packet (tests/accel_ref.py), 4000 rays bit for bit against a freshly built context and the oracle, a frame bit
for bit against the fresh context, the motion snapshot's state.  The builder a sequence starts with goes round the three.
usage: python tools/scene_edit_fuzz.py SEQUENCES STEPS SEED      one line per sequence; stops at the first mismatch and prints the reproducer"""
import os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from gltf_renderer_amd.renderer import Renderer
import oracle.pyoracle as po
from tests import scene_edit_model as sem
from tests.test_gpu_scene_edits import run_sequence


def main():
    sequences, steps, seed0 = (int(x) for x in sys.argv[1:4])
    po.build()
    done = 0
    t0 = time.time()
    for k in range(sequences):
        seed, builder = seed0 + k, sem.BUILDERS[k % len(sem.BUILDERS)]
        try:
            done += run_sequence(Renderer, po, builder, seed, steps)
        except AssertionError as e:
            print("MISMATCH after %d sequences, %d realisations: %s" % (k, done, e))
            print("reproduce: python -c \"from tests.test_gpu_scene_edits import run_sequence; from gltf_renderer_amd.renderer import Renderer; "
                  "import oracle.pyoracle as po; run_sequence(Renderer, po, %d, %d, %d)\"" % (builder, seed, steps))
            return 1
    print("%d sequences, %d realisations, 0 mismatches, %.1f s" % (sequences, done, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
