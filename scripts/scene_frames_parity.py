#!/usr/bin/env python3
"""Every scene driver once on one small scene, a sha256 per result: the record behind profiles/scene_frames/parity.json.

    WEBSPLAT_LIB=<a build's libwebsplat_hip.so> python scripts/scene_frames_parity.py run OUT.json
    python scripts/scene_frames_parity.py merge PARENT.json TREE.json profiles/scene_frames/parity.json

`run` is one process per library (WEBSPLAT_LIB unset: this tree's).  The scene is tests/test_gpu_evaluate.py's: 2 000 Gaussians,
three orbit cameras of 160 x 120, one of them named with the extension in capitals; image b is a pruned copy's parent (ref) or
PNGs of 96 x 72 (gt_dir).  `merge` puts two runs side by side and fails unless they are equal row for row."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-splat_amd"))

N, VIEW, SMALL = 2_000, (160, 120), (96, 72)


def digest(x, h=None):
    import numpy as np
    top = h is None
    h = h or hashlib.sha256()
    if isinstance(x, np.ndarray):
        h.update(str((x.dtype.str, x.shape)).encode())
        h.update(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, (bytes, bytearray)):
        h.update(bytes(x))
    elif isinstance(x, dict):
        for k in sorted(x):
            h.update(str(k).encode())
            digest(x[k], h)
    elif isinstance(x, (list, tuple)):
        for v in x:
            digest(v, h)
    else:
        h.update(repr(x).encode())
    return h.hexdigest() if top else None


def run(out_path):
    import numpy as np
    import websplat as ws
    from websplat import synth

    rows = []

    def row(name, value):
        rows.append({"result": name, "sha256": digest(value)})
        print(f"{rows[-1]['sha256']}  {name}", flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        c = ws.Context(0, ws.config_from_env({}))
        full = synth.scene_c1(n=N, seed=0)
        keep = np.arange(N) % 3 != 2   # every third Gaussian dropped: the pruned cloud against its parent
        ply, sub_ply, cj, gt = (os.path.join(tmp, n) for n in ("parent.ply", "pruned.ply", "cameras.json", "gt"))
        synth.write_ply(ply, full)
        synth.write_ply(sub_ply, full[keep])
        cams = synth.orbit_cameras(3, VIEW[0], VIEW[1], 150.0, 150.0, radius=3.0, height_off=0.4)
        cams[1].img_name = "view_b.PNG"
        synth.write_cameras_json(cj, cams)
        os.mkdir(gt)
        rng = np.random.default_rng(11)
        for cam in cams:
            img = rng.integers(0, 256, size=(SMALL[1], SMALL[0], 4), dtype=np.uint8)
            img[..., 3] = 255
            ws.write_png(os.path.join(gt, cam.img_name if cam.img_name.lower().endswith(".png") else cam.img_name + ".png"), img)
        parent, pc = ws.PointCloud.load(c, ply), ws.PointCloud.load(c, sub_ply)
        scene = ws.Scene.from_json(cj)
        n = pc.num_points()
        forms = (("ref", dict(ref=parent)), ("gt", dict(gt_dir=gt)))

        out = os.path.join(tmp, "views")
        for split in ("train", "test"):
            count = ws.render_views(c, pc, scene, split, out)
            names = sorted(os.listdir(os.path.join(out, split)))
            row(f"render_views {split}: {count} PNG files", [(nm, open(os.path.join(out, split, nm), "rb").read()) for nm in names])

        for form, kw in forms:
            m = ws.Metrics(c, 6)
            for quantize in (False, True):
                ws.evaluate_scene(c, pc, scene, None, m, quantize_u8=quantize, **kw)
            row(f"evaluate_scene {form}: records", [sorted(r.items()) for r in m.download()])
            m.close()

        acc = ws.Contrib(c, n)
        for split in ("train", "test"):
            ws.accumulate_contrib_scene(c, pc, scene, split, acc)
        row("accumulate_contrib_scene: download", acc.download())
        acc.close()

        for kind in ("sq", "abs"):
            effect, weight = ws.Contrib(c, n), ws.Contrib(c, n)
            ws.accumulate_removal_scene(c, pc, scene, "train", effect, weight, kind=kind)
            row(f"accumulate_removal_scene {kind}: effect, weight", [effect.download(), weight.download()])
            effect.close()
            weight.close()

        for form, kw in forms:
            for kind in ("sq", "abs", "dssim"):
                err, weight = ws.Contrib(c, n), ws.Contrib(c, n)
                ws.accumulate_error_scene(c, pc, scene, None, err, weight, kind=kind, **kw)
                row(f"accumulate_error_scene {form} {kind}: err, weight", [err.download(), weight.download()])
                err.close()
                weight.close()
            for kind in ("sq", "abs"):
                grad = ws.Grad(c, n)
                ws.accumulate_gradient_scene(c, pc, scene, None, grad, kind=kind, opacity_scale=0.25, **kw)
                row(f"accumulate_gradient_scene {form} {kind}: download", grad.download())
                grad.close()

        exe = os.path.join(os.path.dirname(os.path.dirname(ws.LIB_PATH)), "bin", "websplat_evaluate")
        for form, opt in (("ref", ["--ref", ply]), ("gt", ["--gt", gt])):
            for split in ("train", "test"):
                p = subprocess.run([exe, sub_ply, cj, *opt, "--split", split, "--blame", "7", "--removal", "7", "--gradient", "7", "--refit", "2",
                                    "--views-per-step", "1"], capture_output=True, timeout=300)
                assert p.returncode == 0, p.stderr.decode()
                text = p.stdout.decode()
                assert all(t in text for t in ("mean over", "blame (", "removal (", "gradient (", "after refit"))
                row(f"websplat_evaluate {form} {split}: all four tables and the refit", p.stdout)

        for form, kw in forms:   # (last: the refit changes its cloud)
            fit_pc = ws.PointCloud.load(c, sub_ply)
            fit = ws.Refit(c, fit_pc)
            steps = ws.refit_scene(c, fit_pc, scene, None, fit, epochs=2, views_per_step=2, **kw)
            row(f"refit_scene {form}: {steps} steps, refit state, cloud", [fit.download(), fit_pc.download()])
            fit.close()
            fit_pc.close()

        scene.close()
        pc.close()
        parent.close()
        c.close()
        with open(out_path, "w") as f:
            json.dump({"library": os.path.relpath(ws.LIB_PATH, ROOT), "rows": rows}, f, indent=1)


def merge(parent_path, tree_path, out_path):
    a, b = (json.load(open(p)) for p in (parent_path, tree_path))
    assert [r["result"] for r in a["rows"]] == [r["result"] for r in b["rows"]], "the two runs list different results"
    rows = [{"result": x["result"], "parent": x["sha256"], "this_tree": y["sha256"], "equal": x["sha256"] == y["sha256"]}
            for x, y in zip(a["rows"], b["rows"])]
    with open(out_path, "w") as f:
        json.dump({"made_by": "scripts/scene_frames_parity.py, one process per library", "parent_library": a["library"],
                   "this_tree_library": b["library"], "all_equal": all(r["equal"] for r in rows), "rows": rows}, f, indent=1)
    return 0 if all(r["equal"] for r in rows) else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "merge":
        sys.exit(merge(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
