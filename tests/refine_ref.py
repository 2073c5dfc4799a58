"""The pose composition at the end of the reference's refine worker (refineWorker_DoWork, LiveScanServer/MainWindowForm.cs:382-410), restated
in numpy: what lsnRefineComposePoses must give, bit for bit.

Every operation is one f32 operation, in the order the C# loops perform them (a product is rounded before it is added), and the
rotation is updated IN PLACE: row j of worldTransforms[i].R is overwritten while the rows behind it are still to be computed from the
matrix, so from the second row on the sums read a mixture of old and new entries.  With an orthogonal R the mixture differs from
Rs^T * R in the last bits at most; with any other matrix it shows.  (Test infrastructure: nothing under livescan3d_amd/ imports this.)"""
import numpy as np

F = np.float32


def compose_poses(Rs, Ts, world_R=None, world_t=None, camera_R=None, camera_t=None):
    """Rs [n,3,3] (row-major, as ICP leaves them) and Ts [n,3]: the accumulated ICP poses.  Returns updated copies
    (world_R, world_t, camera_R, camera_t); a pair that is not given stays None.  Without the world pair the camera rotations stay as they
    are: the C# copies into them what it computed from the world rotation."""
    Rs = np.asarray(Rs, dtype=F).reshape(-1, 9)
    Ts = np.asarray(Ts, dtype=F).reshape(-1, 3)
    n = len(Ts)
    world = world_R is not None and world_t is not None
    camera = camera_R is not None and camera_t is not None
    wR = np.array(world_R, dtype=F).reshape(n, 3, 3) if world else None
    wt = np.array(world_t, dtype=F).reshape(n, 3) if world else None
    cR = np.array(camera_R, dtype=F).reshape(n, 3, 3) if camera else None
    ct = np.array(camera_t, dtype=F).reshape(n, 3) if camera else None
    for i in range(n):
        for j in range(3):
            if world:
                temp = F(0)
                for k in range(3):
                    temp = F(temp + F(Ts[i, k] * wR[i, k, j]))        # :390
                wt[i, j] = F(wt[i, j] + temp)                          # :393
            if camera:
                ct[i, j] = F(ct[i, j] + Ts[i, j])                      # :394
        if not world:
            continue
        for j in range(3):
            for k in range(3):
                temp = F(0)
                for l in range(3):
                    temp = F(temp + F(Rs[i, l * 3 + j] * wR[i, l, k]))   # :403 -- wR[i] as it is NOW
                wR[i, j, k] = temp                                      # :406
                if camera:
                    cR[i, j, k] = temp                                  # :407
    return wR, wt, cR, ct
