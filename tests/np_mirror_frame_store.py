"""CPU restatement in numpy of what the frame store adds to the match stage (frame_gather in cerebro_amd/csrc/frames.hip,
pose_sets_stored_batch in match.hip; definitions in include/cerebro_hip.h, "frames kept on the device"): the point record of a keypoint, and the
five correspondence sets built FROM RECORDS instead of from the 3-D images.  Everything else is np_mirror_match's."""
from __future__ import annotations

import numpy as np

import np_mirror_match as M


def gather(kp_xy, xyz) -> np.ndarray:
    """-> (n, 4) float32 records: (x, y, z, 1) with the three floats of the keypoint's pixel copied bit for bit, (0, 0, 0, 0) for a
    keypoint outside the image (np_mirror_match._pixel: truncation, (-1, w) maps into [0, w - 1], NaN is outside)"""
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float32)
    inside, x, y = M._pixel(kp, xyz.shape[1], xyz.shape[0])
    rec = np.zeros((len(kp), 4), np.float32)
    rec[inside, :3] = xyz[y[inside], x[inside]]
    rec[inside, 3] = np.float32(1.0)
    return rec


def pose_sets(kp1_xy, kp2_xy, train_idx, inlier, rec_a, rec_b, Kinv) -> dict:
    """np_mirror_match.pose_sets with the records of the two frames in place of their images: the point of keypoint i of a is
    rec_a[i, :3], of keypoint t of b rec_b[t, :3]; in_a / in_b are the flags"""
    kp1 = np.ascontiguousarray(kp1_xy, np.float32).reshape(-1, 2)
    kp2 = np.ascontiguousarray(kp2_xy, np.float32).reshape(-1, 2)
    q = np.nonzero(np.asarray(inlier) != 0)[0]
    t = np.asarray(train_idx, np.int64)[q]
    pa, pb = kp1[q], kp2[t]
    ra, rb = np.asarray(rec_a, np.float32)[q], np.asarray(rec_b, np.float32)[t]
    in_a, in_b = ra[:, 3] != 0, rb[:, 3] != 0
    Pa, Pb = ra[:, :3].astype(np.float64), rb[:, :3].astype(np.float64)
    za = in_a & M.depth_ok(ra[:, 2])
    zb = in_b & M.depth_ok(rb[:, 2])
    uv, uv_d = pa.astype(np.float64), pb.astype(np.float64)
    na = M.normalise_pixels(Kinv, uv[:, 0], uv[:, 1])
    nb = M.normalise_pixels(Kinv, uv_d[:, 0], uv_d[:, 1])
    both = za & zb
    out = dict(uv=uv, uv_d=uv_d, match_query_idx=q.astype(np.int32), match_train_idx=t.astype(np.int32),
               X_ab=Pa[za], uvn_ab=nb[za], X_ba=Pb[zb], uvn_ba=na[zb], A_3d3d=Pa[both], B_3d3d=Pb[both])
    out["summary"] = dict(n_matches_gms=len(q), n_3d2d_ab=int(za.sum()), n_3d2d_ba=int(zb.sum()), n_3d3d=int(both.sum()),
                          n_out_of_image=int((~in_a | ~in_b).sum()))
    return out


def stored(frame: dict) -> dict:
    """what the store keeps of a frame: descriptors, keypoints, records and the image size"""
    h, w = frame["xyz"].shape[:2]
    return dict(desc=frame["desc"], kp=frame["kp"], rec=gather(frame["kp"], frame["xyz"]), size=(w, h))


def match_pair(sa: dict, sb: dict, Kinv) -> dict:
    """np_mirror_match.match_pair on two stored() frames"""
    n1, n2 = len(sa["kp"]), len(sb["kp"])
    empty = dict(n_matches_all=0, n_matches_gms=0, n_3d2d_ab=0, n_3d2d_ba=0, n_3d3d=0, n_out_of_image=0)
    if n1 == 0 or n2 == 0:
        return dict(summary=empty, train_idx=np.zeros(0, np.int32), distance=np.zeros(0, np.int32), inlier=np.zeros(0, np.uint8))
    tidx, dist = M.orb_bf_match(sa["desc"], sb["desc"])
    inl = M.gms_filter(sa["kp"], sa["size"], sb["kp"], sb["size"], np.arange(n1), tidx)
    out = pose_sets(sa["kp"], sb["kp"], tidx, inl, sa["rec"], sb["rec"], Kinv)
    out["summary"]["n_matches_all"] = n1
    out.update(train_idx=tidx, distance=dist, inlier=inl)
    return out
