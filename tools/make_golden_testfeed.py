"""BUILD CONTAINER ONLY: run the reference's OWN test-phase dataset — FundusSegmentation(phase='test', state='prediction',
transform=Compose([Resize(256), Normalize_tf(), ToTensor()]), label='OD'), what test_visulization.py:100-110 feeds its loader with — on
the synthetic PNG tree of oracle/fundus_tree.py and record what it hands out -> tests/golden/testfeed.npz.

Recorded per domain d (its test split alone): `d<d>_names` the file names in index order, `d<d>_od_<i>` / `d<d>_oc_<i>` the
`original_od` / `original_oc` label of sample i as uint8, `d<d>_image_sha256` the SHA-256 of each normalised image's fp32 bytes
([3,256,256], C order) — the decoded pixels themselves are pinned by dataset.npz already.  Names, numbers and digests only; no
reference code.  The reference is imported through oracle.ref_import (its custom_transforms wants the cv2 shim)."""
import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT]
from oracle import ref_import  # noqa: E402
from oracle.fundus_tree import make_tree  # noqa: E402

DOMAINS = (1, 2, 3, 4)


class Compose:
    """torchvision.transforms.Compose (not installed): the transforms in order."""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


def main():
    tr = ref_import.load_transforms()
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    import fundus_dataloader as DL
    sys.path.remove(ref_import.REFERENCE_ROOT)
    assert os.path.dirname(os.path.abspath(DL.__file__)) == os.path.abspath(ref_import.REFERENCE_ROOT)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        make_tree(tmp, seed=5)
        for d in DOMAINS:
            ds = DL.FundusSegmentation(base_dir=tmp, phase="test", splitid=[d], state="prediction", label="OD",
                                       transform=Compose([tr.Resize(256), tr.Normalize_tf(), tr.ToTensor()]))
            keys = list(ds.image_pool.keys())
            assert len(keys) == 1, keys
            names, digests = [], []
            for i in range(len(ds)):
                s = ds[i]
                names.append(ds.img_name_pool[keys[0]][i])
                img = s["image"].contiguous().numpy()
                assert img.dtype == np.float32 and img.shape == (3, 256, 256)
                digests.append(hashlib.sha256(img.tobytes()).hexdigest())
                for k in ("od", "oc"):
                    m = s["original_" + k].numpy()
                    assert m.shape[0] == 1 and set(np.unique(m)) <= {0.0, 1.0}
                    out["d%d_%s_%d" % (d, k, i)] = m[0].astype(np.uint8)
            out["d%d_names" % d] = np.array(names)
            out["d%d_image_sha256" % d] = np.array(digests)
    dst = os.path.join(ROOT, "tests", "golden", "testfeed.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
