"""The composition tests/test_gpu_pose_settings_combined.py holds the device to (tests/pose_settings_cases.py), on the CPU: it tells itself
from its two near misses -- the plane stages' normals taken from the filtered frame, and the raw scene throughout -- in the records of
refine_poses, verify_poses and both chains, so a device that mixed the scenes up must fail there."""
import numpy as np
import pytest

import pose_refine_cases as prc
import pose_settings_cases as psx
import pose_verify_cases as pvc
import second_trip_cases as stc


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return stc.Hosts(tmp_path_factory.mktemp("pose_settings"))


def test_the_composition_differs_from_both_near_misses(hosts):
    S = psx.setup()
    st = psx.Settings()
    assert len(S.L.clusters) == 9 and S.offsets == [0, 7, 14, 16] and min(S.n_planted) > 0
    exact = psx.compose(hosts, S, st, S.raw)
    poses, sums, planes, checks = exact
    assert (poses["status"] != prc.NONE).all() and (poses["status"] == prc.NO_OVERLAP).sum() == 4 and (checks["status"] == pvc.OK).any()
    assert sum(int(p[:, 0].astype(bool).sum()) for p in planes) > 20 and (poses["reserved"] == 1).any()              # plane passes ran, in both stages
    scenes = psx.scenes_for(hosts, st, S.raw)
    for f in range(2):
        assert (scenes[f][0] != S.raw[f]).any() and scenes[f][1][..., 3].any()                                       # the filter removed pixels; the raw frame has normals
    rough = psx.rough_records(hosts, S)
    chain, rchain = psx.compose_chain(hosts, S, st, S.raw), psx.compose_rough_chain(hosts, S, st, S.raw, rough)
    assert chain[3].any() and rchain[2].any()
    for variant in (psx.NORMALS_OF_FILTERED, psx.RAW_THROUGHOUT):
        miss = psx.compose(hosts, S, st, S.raw, variant=variant)
        n = int((np.frombuffer(miss[0].tobytes(), np.uint8) != np.frombuffer(poses.tobytes(), np.uint8)).sum())
        differ = [i for i in range(len(poses)) if miss[0][i:i + 1].tobytes() != poses[i:i + 1].tobytes()]
        print("%-32s %d of %d pose records differ (%d bytes), %d verify records" % (variant, len(differ), len(poses), n, sum(
            miss[3][i:i + 1].tobytes() != checks[i:i + 1].tobytes() for i in range(len(poses)))))
        assert len(differ) >= 4, variant
        assert any(not np.array_equal(a, b) for a, b in zip(miss[2], planes)), variant                               # the plane sums themselves
        mchain = psx.compose_chain(hosts, S, st, S.raw, variant=variant)
        assert mchain[1].tobytes() != chain[1].tobytes(), variant
        assert psx.compose_rough_chain(hosts, S, st, S.raw, rough, variant=variant)[0].tobytes() != rchain[0].tobytes(), variant
    assert psx.compose(hosts, S, st, S.raw, variant=psx.RAW_THROUGHOUT)[3].tobytes() != checks.tobytes()             # verify_poses reads the filtered copy too
    # the other scene and other settings of the state sequence give other bytes: a stale copy would show
    assert psx.compose(hosts, S, st, S.other)[0].tobytes() != poses.tobytes()
    assert psx.compose(hosts, S, st.but(scene_filter=(2, 9, 0.5)), S.raw)[0].tobytes() != poses.tobytes()
    assert psx.compose(hosts, S, st.but(normals=(psx.F, psx.F, 20, 640)), S.raw)[0].tobytes() != poses.tobytes()
