"""The labelled test split behind the CLAHE preprocessing: `ClaheTestBatches`, test_run.FundusTestBatches with the stage between its
resize and its normalisation.  A class of its own beside the feed, so that the feed without the stage is the code it was: not one
launch, allocation or byte of its output changes.  programs.open_test_split builds this class when the checkpoint records a `Clahe`
(or --clahe names one) and the plain feed otherwise."""
import numpy as np
import torch

from . import ops
from .input_pipeline import Clahe
from .test_run import FundusTestBatches


class ClaheTestBatches(FundusTestBatches):
    """FundusTestBatches(tree, batch_size, device) with `clahe`, an `input_pipeline.Clahe`: iterating yields the same tuples — (image
    [B,3,S,S] fp32, original_od, original_oc [B,1,h,w] fp32, names), labels and names exactly the plain feed's — with the image taken
    through resize (on the host, Pillow's, as in host_sample), then `ops.clahe` and `ops.image_finish` on the device; image_finish
    equals host_sample's normalisation bit for bit, so the image is `clahe_host` of the resized bytes, `/ 127.5 - 1`.  For a checkpoint
    trained under the same Clahe (its "clahe" entry); `triples()` is what TrainRun(val_batches=...) takes, and `clahe_record()` what it
    compares with its training feed's.  host_sample / host_batch stay the plain feed's: the stage runs on the device only."""

    def __init__(self, tree, batch_size, device="cuda", clahe=None):
        FundusTestBatches.__init__(self, tree, batch_size, device)
        if not isinstance(clahe, Clahe):
            raise ValueError("ClaheTestBatches needs an input_pipeline.Clahe (got %r); without the stage use FundusTestBatches" % (clahe,))
        clahe.check_size(self.size, self.size)
        self.clahe = clahe

    def clahe_record(self):
        return self.clahe.record()

    def host_u8(self, i):
        """-> the resized picture [S,S,3] uint8: what host_sample normalises, and what the device equalises first."""
        return np.array(self.images[i].resize((self.size, self.size)))

    def __iter__(self):
        for b in range(len(self)):
            # (of host_batch the masks, the names and the label-size check are used; the pictures go up as bytes)
            _, mask, names = self.host_batch(b)
            od, oc = ops.label_thresholds(torch.from_numpy(mask).to(self.device))
            idx = range(b * self.batch_size, min((b + 1) * self.batch_size, len(self.images)))
            u8 = torch.from_numpy(np.ascontiguousarray(np.stack([self.host_u8(i) for i in idx]))).to(self.device)
            yield ops.image_finish(ops.clahe(u8, self.clahe)), od, oc, names
