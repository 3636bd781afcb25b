"""The two scenes of the PPFEstimator tests, built on the host so that the GPU test (tests/test_gpu_ppf_estimator.py) and the
restatement chain without a GPU (tests/test_ppf_train.py) see the same inputs, and that chain itself: train with
tests/cpp/ppf_train_ref.c, prepare the scene with the restatements of the normals, the voxel sample and the boundary detection,
vote with tests/cpp/ppf_ref.c, cluster / refine / score with tests/cpp/ppf_cluster_ref.c and the ICP restatements.

Scene one is the reference example's shape: the golden mesh (tests/golden/raycast_obj.npz) at its first golden pose, a plane behind
it as clutter, seen by the golden camera at half resolution.  The mesh carries no normals and has a vertex every few
millimetres: calc_normal_relative = 0.05 (7 mm) is the smallest round figure whose ball holds a neighbourhood to estimate a
normal from; the config's 0.01 (1.4 mm) holds hardly a neighbour.
Scene two is the plate with holes of ppf_edge_ref_util in EdgePoints mode.  Its edges come from boundary detection on the DENSE
sample, whose spacing is rel_dense_sample_dist = 0.025 of the diameter, with Hybrid(calc_normal_relative x diameter, pts_num =
20): a disc of 0.06 diameters holds pi (0.06 / 0.025)^2 = 18 dense points, about the 20 the detector asks for.  At 0.03 it holds
4 or 5 and nearly every dense point is flagged an edge (461 of 537), which leaves the vote little to tell rims from faces."""
import os

import numpy as np

import ppf_edge_ref_util as eu
import ppf_ref_util as pu
import raycast_ref_util as ru

OBJ_NORMAL_REL = 0.05
PLATE_NORMAL_REL = 0.06
SEED = 7


def obj_scene_meshes():
    """-> (meshes, poses, camera, the object's pose)"""
    mesh, poses, cam = ru.golden_obj(2)
    T = poses[0]
    centre = T[:3, :3] @ mesh[0].mean(axis=0) + T[:3, 3]
    z = float(centre[2]) + 0.12                     # a plane behind the object, tilted a little, as clutter
    quad = (np.array([[-0.4, -0.3, z], [0.4, -0.3, z + 0.02], [0.4, 0.3, z + 0.05], [-0.4, 0.3, z + 0.03]]) + [centre[0], centre[1], 0.0],
            np.array([[0, 2, 1], [0, 3, 2]], dtype=np.int32))          # (wound to face the camera)
    return [mesh, quad], [T, np.eye(4)], cam, T


def cloud_of(t_hit, cam):
    """the points of a depth map as RayCastRenderer.get_point_cloud forms them: fp32 rays times fp32 t_hit, ascending pixel order"""
    W, H, fx, fy, cx, cy = cam
    d = np.empty((H, W, 3), np.float32)
    d[..., 0] = (((np.arange(W, dtype=np.float64) + 0.5) - cx) / fx).astype(np.float32)[None, :]
    d[..., 1] = (((np.arange(H, dtype=np.float64) + 0.5) - cy) / fy).astype(np.float32)[:, None]
    d[..., 2] = 1.0
    hit = np.isfinite(t_hit)
    return np.ascontiguousarray((d[hit] * t_hit[hit][:, None]).astype(np.float64))


def plate_model():
    pts, nrm, _, _, _ = eu.plate_with_holes(n_side=84, seed=11)
    return np.ascontiguousarray(pts + np.array([0.1, -0.2, 0.3])), nrm


def plate_scene(model, prepared_normals):
    """the posed model with its prepared normals facing a camera at the origin, two units away, in 1 500 points of clutter
    -> (points, normals, the pose)"""
    R = pu.pose(3)[:3, :3]
    mean = prepared_normals.mean(axis=0)
    face = R @ (mean / np.linalg.norm(mean))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -2.0 * face - R @ model.mean(axis=0)
    sp, sn, _ = pu.scene_of(model, prepared_normals, T, 1500, 3)
    return sp, sn, T


def pose_error(pose, T):
    """-> (translation error, rotation angle) of pose against T"""
    dR = pose[:3, :3].T @ T[:3, :3]
    return float(np.linalg.norm(pose[:3, 3] - T[:3, 3])), float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))


# ---- the restatement chain
def normal_consistent(p, n):
    """NormalConsistent (include/misc3d/utils.h:130-144): the same rounded operations in the same order"""
    n = n.copy()
    flip = (p[:, 0] * n[:, 0] + p[:, 1] * n[:, 1]) + p[:, 2] * n[:, 2] > 0.0
    n[flip] = -n[flip]
    s = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    ok = s > 0.0
    n[ok] = n[ok] / np.sqrt(s[ok])[:, None]
    return n


class Chain:
    """the restatements, built once into tmpdir"""

    def __init__(self, tmpdir):
        import fpfh_ref_util as fu
        import icp_ref_util as iu
        import oracle
        import ppf_cluster_ref_util as cu
        import ppf_train_ref_util as tu
        import voxel_ref_util as vu
        os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
        oracle.build()
        self.oracle, self.cu = oracle, cu
        self.train, self.normals, self.voxel = tu.TrainRef(tmpdir), fu.build_ref(tmpdir), vu.build_ref(tmpdir)
        self.ppf, self.pc, self.icp = pu.PpfRef(tmpdir, openmp=True), cu.PcRef(tmpdir), iu.IcpRef(tmpdir)
        self.render = ru.build_ref(tmpdir, openmp=True)

    def edges(self, pts, nrm, radius):
        return np.asarray(self.oracle.detect_boundary_points(np.ascontiguousarray(pts), np.ascontiguousarray(nrm), 2, radius, 20, 90.0)).astype(np.int64)

    def run(self, model, model_normals, scene, scene_normals, normal_rel, edge, score_thresh):
        """Train and Estimate by the contract -> (PcRef.finish's dict, the model info, dict of counts)"""
        t = self.train
        c, e = t.box(model)
        d = t.derive(c, e, 0.05, 0.025, normal_rel)
        n0 = model_normals if model_normals is not None else self.normals.normals(model, 2, d["normal_r"], 30)
        m = t.prepare_model(model, n0, box=(c, e), rel_dense_sample_dist=0.025 if edge else 0.0, calc_normal_relative=normal_rel)
        info, si = m["info"], m["sample_indices"]
        sn = scene_normals if scene_normals is not None else self.normals.normals(scene, 2, normal_rel * info["diameter"], 30)
        sn = normal_consistent(scene, sn)
        s = self.voxel(scene, info["dist_step"], normals=sn)
        num = len(s["points"])
        ref = t.reference_indices(num, int(0.6 * num), SEED)
        me = se = (None, None)
        counts = dict(model_sample=len(si), scene_sample=num)
        if edge:
            di = m["dense_indices"]
            ei = di[self.edges(model[di], m["normals"][di], info["normal_r"])]
            dense = self.voxel(scene, info["dist_step_dense"], normals=sn)
            k = self.edges(dense["points"], dense["normals"], info["normal_r"])
            me = (np.ascontiguousarray(model[ei]), np.ascontiguousarray(m["normals"][ei]))
            se = (np.ascontiguousarray(dense["points"][k]), np.ascontiguousarray(dense["normals"][k]))
            counts.update(model_dense=len(di), model_edges=len(ei), scene_edges=len(k))
        rm = self.ppf.model(np.ascontiguousarray(model[si]), np.ascontiguousarray(m["normals"][si]), info["diameter"], info["r_min"], pu.params(),
                            me[0], me[1])
        raw = rm.vote(s["points"], s["normals"], ref, se[0], se[1])
        cen = rm.table()["centroid"]
        res = self.cu.estimate_ref(self.pc, self.icp, raw["poses"], raw["votes"], np.ascontiguousarray(model[si] - cen), cen, s["points"],
                                   s["normals"], info["dist_step"], 0.05 * info["diameter"], score_thresh=score_thresh,
                                   refine_method="PointToPlane")
        counts.update(raw_poses=len(raw["votes"]))
        return res, info, counts
