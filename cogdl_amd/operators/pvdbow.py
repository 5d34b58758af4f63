"""PV-DBOW training over ragged documents: the trainer behind `gensim.models.doc2vec.Doc2Vec(documents, dm=0, negative=K)`
as the reference's Graph2Vec calls it (cogdl/models/emb/graph2vec.py:99-109): skip-gram with negative sampling whose input
row is the document's vector.

    doc2vec_dbow(doc_ptr, words, num_words, dim, negative, epochs, ...) -> (dv float32 [G, dim], syn1 float32 [num_words, dim])

`doc_ptr` is int64 [G + 1], non-decreasing from 0 to T; `words` int64 [T] with ids in [0, num_words), a negative id is
padding.  Words on the GPU go to the HIP kernel (cogdl_hip_pvdbow_train, csrc/pvdbow.hip: one wave per document, the
document's vector in registers) and the tables stay there; words on the CPU go to the host twin in libcogdl_host.so, and
libcogdl_hip.so is not loaded.  Both run the law of csrc/pvdbow_law.h on top of csrc/sgns_law.h; the subsampling thresholds,
the noise table and the sigmoid table are those of operators/sgns.py.

  * `workers=1` is the serial mode: documents in order on one wave (GPU) or one thread (host); both return the same
    tables, bit for bit, and the same from run to run.  Any other value is the throughput mode: on the GPU, documents go
    in launches of DOCS_IN_FLIGHT documents, in document order; syn1 is updated without locks, so results differ from run
    to run, while a document's vector has one writer.
  * An id >= num_words, a malformed noise table and a doc_ptr that runs backwards or past T raise BackendError and the
    tables are not touched; nothing is read out of bounds.
  * There is no cap on a document's length (below 2^32) and no window.  One wave per document: a batch with one very long
    document is uneven.
"""
import torch

from .. import _lib
from . import sgns
from .sgns import MAX_DIM, MAX_NEGATIVE, exp_table
from .walk import _seed

# Documents per launch of the GPU's throughput mode (0 = the library's default, 8192).
DOCS_IN_FLIGHT = 0

_FLAG_TEXT = ((1, "an id lies outside [0, %d)"), (2, "the noise table is not non-decreasing with a positive last entry (%d ids)"),
              (4, "doc_ptr runs backwards or outside the words (%d ids)"))


def init_tables(num_docs, num_words, dim, seed, device):
    """(dv [G, dim], syn1 [V, dim]) float32: dv[g][d] = (u24(seed; g, d) / 2^24 - 0.5) / dim under the document stream,
    syn1 = 0; equal on both sides."""
    device = torch.device(device)
    dv = torch.empty((num_docs, dim), dtype=torch.float32, device=device)
    syn1 = torch.empty((num_words, dim), dtype=torch.float32, device=device)
    if device.type == "cuda":
        with _lib.on_device(device):
            rc = _lib.hip().cogdl_hip_pvdbow_init(_lib.ptr(dv), num_docs, _lib.ptr(syn1), num_words, dim, seed, _lib.stream_of(dv))
        _lib.check(rc, "doc2vec_dbow (init)")
    else:
        _lib.check_host(_lib.host().cogdl_host_pvdbow_init(_lib.ptr(dv), num_docs, _lib.ptr(syn1), num_words, dim, seed),
                        "doc2vec_dbow (init)")
    return dv, syn1


def doc2vec_dbow(doc_ptr, words, num_words, dim=128, negative=5, epochs=10, alpha=0.025, min_alpha=1e-4, sample=0.0,
                 ns_exponent=0.75, seed=None, workers=0, init=None, tables=None):
    """-> (dv, syn1) on the device of `words`.  `init=(dv, syn1)` continues from tables of the caller's (they are copied,
    not modified).  `tables=(keep, cum)` replaces the tables built from the counts (int64 tensors of uint32 values)."""
    if not torch.is_tensor(words) or words.dtype != torch.long or words.dim() != 1:
        raise ValueError("doc2vec_dbow: words must be an int64 [T] tensor")
    if not torch.is_tensor(doc_ptr) or doc_ptr.dtype != torch.long or doc_ptr.dim() != 1 or doc_ptr.numel() < 1:
        raise ValueError("doc2vec_dbow: doc_ptr must be an int64 [G + 1] tensor")
    num_words, dim, negative, epochs, workers = int(num_words), int(dim), int(negative), int(epochs), int(workers)
    alpha, min_alpha, sample, ns_exponent = float(alpha), float(min_alpha), float(sample), float(ns_exponent)
    if num_words < 1 or num_words > 2 ** 31 - 1:
        raise ValueError("doc2vec_dbow: num_words must be in [1, 2^31) (got %d)" % num_words)
    sgns.check_range("doc2vec_dbow", "dim", dim, MAX_DIM)
    sgns.check_range("doc2vec_dbow", "negative", negative, MAX_NEGATIVE)
    sgns.check_schedule("doc2vec_dbow", epochs, alpha, min_alpha, sample)
    sgns.check_workers("doc2vec_dbow", workers)
    docs_in_flight = int(DOCS_IN_FLIGHT)
    if docs_in_flight < 0:
        raise ValueError("doc2vec_dbow: DOCS_IN_FLIGHT must be >= 0 (got %d)" % docs_in_flight)
    dev = words.device
    g, t = doc_ptr.numel() - 1, words.numel()
    if init is not None:
        sgns.check_init(init, (g, num_words), dim, dev,
                        "doc2vec_dbow: init must be float32 [%d, %d] and [%d, %d] tensors on %s" % (g, dim, num_words, dim, dev))
    sgns.check_tables("doc2vec_dbow", tables, num_words)
    seed = _seed(seed)
    words, doc_ptr = words.contiguous(), doc_ptr.to(dev).contiguous()
    keep, cum = sgns.noise_tables(words, num_words, tables, sample, ns_exponent, dev)
    table = exp_table().to(dev)
    if init is None:
        dv, syn1 = init_tables(g, num_words, dim, seed, dev)
    else:
        dv, syn1 = init[0].clone().contiguous(), init[1].clone().contiguous()
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    if dev.type == "cuda":
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_pvdbow_train(_lib.ptr(doc_ptr), g, _lib.ptr(words), t, num_words, dim, negative, epochs, alpha,
                                                   min_alpha, _lib.ptr(keep), _lib.ptr(cum), _lib.ptr(table), seed, workers,
                                                   docs_in_flight, _lib.ptr(dv), _lib.ptr(syn1), _lib.ptr(flags),
                                                   _lib.stream_of(words))
        _lib.check(rc, "doc2vec_dbow")
    else:
        rc = _lib.host().cogdl_host_pvdbow_train(_lib.ptr(doc_ptr), g, _lib.ptr(words), t, num_words, dim, negative, epochs, alpha,
                                                 min_alpha, _lib.ptr(keep), _lib.ptr(cum), _lib.ptr(table), seed, workers,
                                                 _lib.ptr(dv), _lib.ptr(syn1), _lib.ptr(flags))
        _lib.check_host(rc, "doc2vec_dbow")
    sgns.raise_flags("doc2vec_dbow", flags, _FLAG_TEXT, num_words)
    return dv, syn1
