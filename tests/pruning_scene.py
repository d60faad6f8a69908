"""Scenes for the pruning tests (PruneWeaklyConnectedImages): seeded random track sets over a few image groups, and one
hand-built scene.  tools/gen_golden.py --only pruning runs the reference on the same scenes and records what it does
(tests/golden/pruning_golden.npz), so this file is the single definition of their inputs."""
import numpy as np

from instantsfm_amd.scene.defs import Image, Track

# the committed seeds (tools/gen_golden.py --only pruning picked them from 0-299: at least five that unregister an
# image, five with several clusters, five whose outcome changes when the pairs are ordered by key)
SEEDS = (2, 3, 4, 7, 11, 17, 22, 26, 30, 35, 37, 40, 41, 43, 47, 49, 50, 56, 58, 59, 61, 62, 64, 66)
HAND = "hand"


def random_scene(seed):
    """(M, track_ptr, obs_img): 8-39 images in 1-4 groups; 200-2999 tracks of 1-8 rows, each drawn with replacement
    from one group (3 %: from all images), so there are repeated images and tracks of one or two rows."""
    rng = np.random.default_rng(seed)
    M = int(rng.integers(8, 40))
    G = int(rng.integers(1, 5))
    group = rng.integers(0, G, M)
    rows = []
    for _ in range(int(rng.integers(200, 3000))):
        members = np.flatnonzero(group == rng.integers(0, G))
        if rng.random() < 0.03 or members.size == 0:
            members = np.arange(M)
        rows.append(rng.choice(members, int(rng.integers(1, 9))))
    return (M, *_csr(rows))


def hand_scene():
    """A main ring (images 0-9), a satellite group (10-14) joined to the ring by 12 shared tracks, and two images
    (15, 16) that share 3 tracks each with the ring.  All tracks have 3 rows."""
    rows = []
    for i in range(10):
        rows += [[i, (i + 1) % 10, (i + 2) % 10]] * 40
    for i in range(5):
        rows += [[10 + i, 10 + (i + 1) % 5, 10 + (i + 2) % 5]] * 40
    rows += [[0, 10, 1]] * 12
    rows += [[3, 4, 15]] * 3 + [[16, 6, 7]] * 3
    return (17, *_csr(rows))


def _csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, np.concatenate(rows).astype(np.int32)


def scene(name):
    return hand_scene() if name == HAND else random_scene(int(name))


def names():
    return [str(s) for s in SEEDS] + [HAND]


def as_objects(M, track_ptr, obs_img, image_cls=Image, track_cls=Track):
    """(images, tracks) as the processors take them: every image registered, observations [L, 2] int64 with the row
    number as the feature id, tracks keyed 0, 1, 2 ..."""
    images = [image_cls(id=i, is_registered=True) for i in range(M)]
    tracks = {}
    for t in range(len(track_ptr) - 1):
        img = np.asarray(obs_img[track_ptr[t]:track_ptr[t + 1]], dtype=np.int64)
        tracks[t] = track_cls(id=t, observations=np.stack([img, np.arange(img.size)], 1))
    return images, tracks
