"""
The block pipeline of the consumers of finished batches (grim.em, grim.marginal, grim.match, grim.search): input lines are
cut into blocks, each block is tokenised and imputed as one device batch, and the consumer works where the batch's rows lie.
What the tokenizer or the device cannot answer is noted on the Imputation as `impute_lines_block` notes it.
"""

import os

import numpy as np

from . import _native as nat

# kinds of line the tokenizer keeps off the device -> the reason an unsupported subject is reported with
host_reason = {nat.K_UNSUPPORTED: 5, nat.K_UNSUPPORTED_GL: 8}


def read_lines(lines_or_path):
    """input lines (a list) or the path of an input file -> the lines without their line ends"""
    if isinstance(lines_or_path, (str, bytes, os.PathLike)):
        with open(lines_or_path) as fh:
            return fh.read().splitlines()
    return [l.rstrip("\n") for l in lines_or_path]


def note_unsupported(imputation, bad):
    """a block's unsupported subjects [(line, id, reason)] onto imputation.unsupported, sorted within the block; raises
    when the policy is "raise" -- before the caller formats the block's text or uses its records"""
    from .imputation.impute import UnsupportedSubjects

    imputation.unsupported += sorted(bad)
    if imputation.unsupported and imputation.on_unsupported == "raise":
        raise UnsupportedSubjects(imputation.unsupported)


class Blocks:
    """what the blocks of one call share: the batch parameters (`outputs`: configuration keys forced, as output_MUUG=True), the
    prior specification, the context and the graph on the device"""

    def __init__(self, imputation, config, planb, em_mr, em, **outputs):
        self.imputation = imputation
        self.planb = config["planb"] if planb is None else planb
        self.params = imputation._params(dict(config, **outputs), self.planb, em_mr, em)
        self.ps, self._counts = nat.prior_spec(config["priority"], imputation.unk_priors, imputation.count_by_prob)
        self.ctx = nat.default_context(imputation.device)
        self.dgraph = imputation.netGraph.device(self.ctx)

    def block(self, lines, lo=0):
        """an open Block of `lines`, the first of which is line `lo` of the input; the caller closes it"""
        return Block(self, lines, lo)

    def cut(self, lines, block_lines, first=0):
        """`lines` in blocks of `block_lines`: yields each as an open Block and closes it when the caller comes back for the next
        (or closes the generator); `first`: the input line `lines` begins at"""
        for lo in range(0, len(lines), block_lines):
            block = self.block(lines[lo:lo + block_lines], first + lo)
            try:
                yield block
            finally:
                block.close()


class Block:
    """a block of input lines tokenised and imputed as one device batch; `batch` is None when no line reached the device"""

    def __init__(self, shared, lines, lo):
        imputation = shared.imputation
        self.lo = lo
        self.batch = None
        self._records = None
        self.parsed = nat.Parsed(imputation.netGraph.adict, "".join(l + "\n" for l in lines).encode(), shared.planb)
        try:
            kinds = self.parsed.kinds()
            dev = self.parsed.dev_index()
            self.bad = [(lo + int(j), self.parsed.subject_id(int(j)), host_reason[int(kinds[j])])
                        for j in np.flatnonzero(np.isin(kinds, list(host_reason)))]
            on_dev = np.flatnonzero(kinds == nat.K_DEVICE)
            self.line_of = np.zeros(self.parsed.n_subjects, dtype=np.int64)  # device subject -> line of the block
            self.line_of[dev[on_dev]] = on_dev
            subj = self.parsed.subjects()
            if len(subj):
                priors = nat.prior_matrices(shared.ps, imputation.populations, self.parsed.races())
                self.batch = nat.DeviceBatch(shared.ctx, shared.dgraph, shared.params, subj, self.parsed.tokens(), priors)
                self.batch.run()
        except BaseException:
            self.close()
            raise

    def records(self):
        """the batch's result records (res, rows), fetched once"""
        if self._records is None:
            self._records = self.batch.results()
        return self._records

    def unsupported(self, res=None):
        """[(line, id, reason)] of the subjects the device could not answer; `res`: result records that carry the batch's
        status and reason (None: the batch's own, fetched)"""
        if res is None:
            res, _ = self.records()
        return [(self.lo + int(self.line_of[i]), self.parsed.subject_id(int(self.line_of[i])), int(res[i]["reason"]))
                for i in np.flatnonzero(res["status"] == nat.ST_UNSUPPORTED)]

    def close(self):
        if self.batch is not None:
            self.batch.close()
            self.batch = None
        self.parsed.close()
