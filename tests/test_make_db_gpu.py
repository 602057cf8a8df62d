"""make_db drop-in on the GPU with the synthetic language model: the batched path
(fingerprint_batch) must equal queue_cpu protein by protein, which in turn is checked against the
CPU oracles; files must have the reference layout; one GPU and two worker processes must write
identical files."""

import os

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu
FIX = os.path.join(gu.GOLD, 'ref_fixtures')


def test_fingerprint_batch_equals_queue_cpu_and_oracle():
    import dctdomain_amd as dd
    from dctdomain_amd import make_db
    from dctdomain_amd.embedding import Batch, SyntheticModel
    from oracle import contacts_oracle as co
    from oracle import dct_oracle as orc
    seqs = []
    with open(os.path.join(FIX, 'example.fasta')) as fh:
        for line in fh:
            if line.startswith('>'):
                seqs.append([line.split()[0][1:], ''])
            else:
                seqs[-1][1] += line.strip()
    dev = torch.device('cuda', 0)
    model = SyntheticModel()
    model.to_device(dev)

    def embed_all():
        out = []
        for pid, seq in seqs:
            b = Batch([(pid, seq)], model, dev)
            b.embed_batch([15, 21], 500)
            e = b.embeds[0]
            out.append(dd.Fingerprint(pid=e.pid, seq=e.seq, embed=e.embed, contacts=e.contacts))
        return out

    one_by_one = [make_db.queue_cpu(fp) for fp in embed_all()]
    batched = make_db.fingerprint_batch(embed_all(), threads=4)
    n_multi = 0
    for a, b in zip(one_by_one, batched):
        assert a.domains == b.domains
        for k in a.domains:
            np.testing.assert_array_equal(a.quants[k], b.quants[k])
        n_multi += len(a.domains) > 1
        # CPU chain: oracle top-k -> reference RecCut binary -> oracle quantize
        ct = a.contacts.cpu().numpy()
        ci, cj, cv = co.top_contacts(ct, 2.6)
        if os.path.exists(co.REF_BIN):
            rc, out = co.run_ref_binary(co.ce_text(a.pid, a.seq, ci, cj, cv), a.pid)
            assert rc == 0 and co.parse_reccut(out, len(a.seq)) == a.domains
        q = orc.quantize([a.embed[15].cpu().numpy(), a.embed[21].cpu().numpy()], a.domains, [3, 80, 3, 80])
        for k in q:
            np.testing.assert_array_equal(a.quants[k], q[k])
    assert n_multi >= 3


def _run(tmp_path, name, extra):
    from dctdomain_amd import make_db
    dbfile = str(tmp_path / name)
    make_db.main(['--fafile', os.path.join(FIX, 'example.fasta'), '--dbfile', dbfile, '--model', 'synthetic',
                  '--cpu', '4', '--out', str(tmp_path / f'{name}.log')] + extra)
    return dbfile


def test_cli_outputs_and_two_workers(tmp_path):
    a = _run(tmp_path, 'one', [])
    za = np.load(a + '-dct.npz')
    assert za['sid'].shape == (8,) and za['idx'][0] == 0 and za['idx'][-1] == za['dct'].shape[0]
    assert za['dct'].dtype == np.int8 and za['dct'].shape[1] == 480 and za['idx'].dtype == np.int64
    rows = za['dct'].reshape(-1, 6, 80)
    assert ((rows == 127).sum(axis=2) == 1).all() and ((rows == 0).sum(axis=2) >= 1).all()
    dom_lines = open(a + '.dom').read().strip().split('\n')
    assert len(dom_lines) == 8 and all(len(l.split()) == 3 for l in dom_lines)
    assert os.path.exists(a + '.index') and os.path.exists(a + '.db')
    assert 'Fingerprinted' in open(str(tmp_path / 'one.log')).read()
    # resume: a second run over the finished database fingerprints nothing new
    from dctdomain_amd.database import Database
    db = Database(a + '.db')
    assert db.pending() == []
    db.close()
    # two worker processes (both on the one visible GPU here) write the same files
    b = _run(tmp_path, 'two', ['--gpu', '2', '--flush', '3'])
    zb = np.load(b + '-dct.npz')
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k])
    assert open(a + '.dom').read() == open(b + '.dom').read()


def test_config5_scale_build_two_workers_against_one_and_oracle(tmp_path):
    """BASELINE config 5, scaled to one GPU box: 5 200 proteins with pfam-like lengths (81..1330) through the
    make_db drop-in -- two worker processes against one (identical files: the single writer commits every flush in
    sequence order), then a sample of proteins recomputed by the CPU chain (oracle top-k -> the reference's RecCut
    binary when it is there -> oracle quantize) against the rows of the written -dct.npz."""
    from dctdomain_amd import make_db
    from dctdomain_amd.embedding import Batch, SyntheticModel
    from oracle import contacts_oracle as co
    from oracle import dct_oracle as orc
    rng = np.random.default_rng(55)
    n_prot = 5200
    lengths = np.clip(rng.gamma(2.2, 170.0, size=n_prot).astype(np.int64), 81, 1330)
    fa = str(tmp_path / 'c5.fasta')
    seqs = {}
    with open(fa, 'w') as fh:
        for i, L in enumerate(lengths):
            s = ''.join('ACDEFGHIKLMNPQRSTVWY'[int(v)] for v in rng.integers(0, 20, size=int(L)))
            seqs[f'P{i:05d}'] = s
            fh.write(f'>P{i:05d} synthetic\n{s}\n')

    def build(name, extra):
        dbfile = str(tmp_path / name)
        make_db.main(['--fafile', fa, '--dbfile', dbfile, '--model', 'synthetic', '--cpu', '8', '--noindex',
                      '--flush', '512', '--out', str(tmp_path / f'{name}.log')] + extra)
        return dbfile

    two = build('two', ['--gpu', '2'])
    one = build('one', [])
    za, zb = np.load(one + '-dct.npz'), np.load(two + '-dct.npz')
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k])
    assert open(one + '.dom').read() == open(two + '.dom').read()
    assert za['sid'].shape == (n_prot,) and za['dct'].shape[1] == 480 and za['dct'].shape[0] == za['idx'][-1]
    assert za['dct'].shape[0] > 2 * n_prot                      # mostly multi-domain: parts + whole protein
    # table order = ascending length (stable), whatever the number of workers
    assert list(za['sid']) == sorted(seqs, key=lambda p: len(seqs[p]))
    rows = za['dct'].reshape(-1, 6, 80)
    assert ((rows == 127).sum(axis=2) == 1).all() and ((rows == 0).sum(axis=2) >= 1).all()
    # the database is complete and resumable: nothing pending, fpcount = rows per protein
    from dctdomain_amd.database import Database
    db = Database(two + '.db')
    assert db.pending() == []
    db.close()

    # sample: CPU chain on the same embeddings
    dev = torch.device('cuda', 0)
    model = SyntheticModel()
    model.to_device(dev)
    sid = list(za['sid'])
    n_multi = 0
    for pid in [sid[i] for i in (0, 7, 601, 1999, 2600, 3333, 4100, 4800, 5100, 5199)]:
        b = Batch([(pid, seqs[pid])], model, dev)
        b.embed_batch([15, 21], 500)
        e = b.embeds[0]
        ct = e.contacts.cpu().numpy()
        ci, cj, cv = co.top_contacts(ct, 2.6)
        k = sid.index(pid)
        doms = [str(d) for d in za['dom'][za['idx'][k]:za['idx'][k + 1]]]
        if os.path.exists(co.REF_BIN):
            rc, out = co.run_ref_binary(co.ce_text(pid, seqs[pid], ci, cj, cv), pid)
            assert rc == 0 and co.parse_reccut(out, len(seqs[pid])) == doms
        q = orc.quantize([e.embed[15].cpu().numpy(), e.embed[21].cpu().numpy()], doms, [3, 80, 3, 80])
        assert list(q) == doms
        for r, key in enumerate(doms):
            np.testing.assert_array_equal(za['dct'][za['idx'][k] + r].astype(np.int64), q[key], err_msg=f'{pid} {key}')
        n_multi += len(doms) > 1
    assert n_multi >= 5


def test_constant_channel_is_reported_by_the_drop_in(tmp_path, monkeypatch):
    """the one documented deviation from the reference -- an exactly constant channel gives 0/0 -> the
    all-zero (layer, domain) block at EVERY domain length, where scipy's pocketfft scales round-off noise at 225 of the
    lengths 3..2000 (tests/golden/fence_golden.json) -- must not be silent for a user of the drop-in: make_db logs a
    warning naming the proteins (into --out), Fingerprint.quantize does the same for its one protein."""
    import json
    import logging
    import dctdomain_amd as dd
    from dctdomain_amd import make_db
    from dctdomain_amd.embedding import SyntheticModel
    noisy_lengths = set(json.load(open(os.path.join(gu.GOLD, 'fence_golden.json')))['const']['noisy_L'])
    assert len(noisy_lengths) == 225

    class OneDeadChannel(SyntheticModel):
        """layer 15, channel 7 carries the same value at every residue (a dead unit of the language model)."""
        def esm_encoder(self, tokens, repr_layers=None, return_contacts=True):
            out = super().esm_encoder(tokens, repr_layers, return_contacts)
            out['representations'][15][..., 7] = 1.5
            return out

    def load_model(name, device):
        m = OneDeadChannel()
        m.to_device(device)
        return m

    monkeypatch.setattr(make_db, 'load_model', load_model)
    L = min(n for n in noisy_lengths if n >= 90)               # a length at which the reference would NOT give the 0 block
    rng = np.random.default_rng(3)
    fa = str(tmp_path / 'dead.fasta')
    with open(fa, 'w') as fh:
        for pid, n in (('NOISY', L), ('OTHER', 130)):
            fh.write(f'>{pid} synthetic\n' + ''.join('ACDEFGHIKLMNPQRSTVWY'[int(v)] for v in rng.integers(0, 20, size=n)) + '\n')
    dbfile, log = str(tmp_path / 'dead'), str(tmp_path / 'dead.log')
    make_db.main(['--fafile', fa, '--dbfile', dbfile, '--model', 'synthetic', '--cpu', '2', '--noindex', '--out', log])
    text = open(log).read()
    assert 'constant channel in' in text and 'NOISY' in text and 'OTHER' in text and '225 of the lengths' in text
    z = np.load(dbfile + '-dct.npz')
    assert (z['dct'][:, :240] == 0).all()                       # layer 15: every (domain) block is the 0 block
    rows = z['dct'][:, 240:].reshape(-1, 3, 80)                 # layer 21 is untouched
    assert ((rows == 127).sum(axis=2) == 1).all()
    # the class itself, one protein per call (own handler: make_db's --out replaced the root logger's handlers)
    seen = []
    grab = logging.Handler()
    grab.emit = lambda record: seen.append(record.getMessage())
    logging.getLogger().addHandler(grab)
    try:
        x = np.random.default_rng(4).standard_normal((L, 640)).astype(np.float32)
        x[:, 11] = -0.25
        fp = dd.Fingerprint(pid='ONE', seq='A' * L, embed={0: x}, domains=[f'1-{L}'])
        fp.quantize([3, 80])
        assert any('constant channel in ONE' in m for m in seen)
        assert (fp.quants[f'1-{L}'] == 0).all()
        del seen[:]
        y = x.copy()
        y[:, 11] = x[:, 12]
        fp = dd.Fingerprint(pid='FINE', seq='A' * L, embed={0: y}, domains=[f'1-{L}'])
        fp.quantize([3, 80])
        assert not any('constant channel' in m for m in seen)
    finally:
        logging.getLogger().removeHandler(grab)


def _embedded(lens, seed=5, dim=640):
    import dctdomain_amd as dd
    from dctdomain_amd.embedding import Batch, SyntheticModel
    rng = np.random.default_rng(seed)
    aa = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)
    dev = torch.device('cuda', 0)
    model = SyntheticModel(dim=dim)
    model.to_device(dev)
    out = []
    for i, L in enumerate(lens):
        b = Batch([(f'p{i:04d}', aa[rng.integers(0, 20, size=int(L))].tobytes().decode())], model, dev)
        b.embed_batch([15, 21], 500)
        e = b.embeds[0]
        out.append((e.pid, e.seq, e.embed, e.contacts))
    fresh = lambda: [dd.Fingerprint(pid=p, seq=s, embed=e, contacts=c) for p, s, e, c in out]
    return fresh


def _assert_same_as_queue_cpu(got, ref):
    """Objects of a flush against ``queue_cpu`` run protein by protein: domains, key order, int64 quants."""
    for fa, fb in zip(got, ref):
        assert fa.domains == fb.domains and list(fa.quants) == list(fb.quants) == fa.domains, fa.pid
        for k in fa.domains:
            assert fa.quants[k].dtype == np.int64 == np.asarray(fb.quants[k]).dtype
            np.testing.assert_array_equal(fa.quants[k], fb.quants[k], err_msg=f'{fa.pid} {k}')


def test_two_phase_flush_equals_queue_cpu_and_the_records():
    """The flush as make_db runs it (geometry in one pass, strings + pieces from the cutter's integers, objects laid out while the
    kernels run) against queue_cpu run protein by protein on fresh objects (the host RecCut library and the one-protein
    quantize), object for object; the writer's records against both; proteins the GPU cutter hands back (L > 2 048),
    single-domain and 30-residue proteins inside."""
    from dctdomain_amd import make_db, reccut
    rng = np.random.default_rng(3)
    lens = np.clip(rng.gamma(2.2, 150.0, size=160).astype(int), 30, 1500).tolist() + [30, 31, 45, 2100, 640, 2300, 97]
    fresh = _embedded(lens)
    a = make_db.fingerprint_batch(fresh(), threads=4)
    assert make_db.LAST_PATH[0] == 'flush' and sorted(reccut.LAST.host_redo) == [163, 165]
    b = [make_db.queue_cpu(fp) for fp in fresh()]
    recs = make_db.flush_records(fresh(), threads=4)
    assert make_db.LAST_PATH[0] == 'flush'
    _assert_same_as_queue_cpu(a, b)
    n_multi = 0
    for fa, fb, ra in zip(a, b, recs):
        n_multi += len(fa.domains) > 1
        assert ra[0] == fb.pid == fa.pid and ra[1] == fb.domains == fa.domains
        assert ra[2].dtype == np.int8 and ra[2].shape == (len(fa.domains), 480)
        np.testing.assert_array_equal(ra[2].astype(np.int64), np.array([fb.quants[k] for k in fb.domains]))
        np.testing.assert_array_equal(ra[2].astype(np.int64), np.array([fa.quants[k] for k in fa.domains]))
    assert n_multi >= 100
    np.testing.assert_array_equal(make_db._records(a)[7][2], recs[7][2])


def _every_other_row_strided(fps):
    for fp in fps[::2]:
        wide = {}
        for k, v in fp.embed.items():
            w = torch.zeros((v.shape[0], v.shape[1] + 64), dtype=v.dtype, device=v.device)
            w[:, :v.shape[1]] = v
            wide[k] = w[:, :v.shape[1]]
        fp.embed = wide


def _mixed(fps):
    for fp in fps[len(fps) // 2:]:
        fp.contacts = fp.contacts.cpu().numpy()
        fp.embed = {k: v.cpu().numpy() for k, v in fp.embed.items()}


def _embed_as(f):
    return lambda fps: [setattr(fp, 'embed', {k: f(v) for k, v in fp.embed.items()}) for fp in fps]


def _maps_as(f):
    return lambda fps: [setattr(fp, 'contacts', f(fp.contacts)) for fp in fps]


#: every input kind the flush converts (or builds the piece table from strings for), and those it takes as they are
_INPUT_KINDS = {
    'numpy embeddings': (_embed_as(lambda v: v.cpu().numpy()), 'converted'),
    'cpu embeddings': (_embed_as(lambda v: v.cpu()), 'converted'),
    'numpy maps': (_maps_as(lambda c: c.cpu().numpy()), 'converted'),
    'cpu maps': (_maps_as(lambda c: c.cpu()), 'converted'),
    'flat maps': (_maps_as(lambda c: c.reshape(-1)), 'converted'),
    'transposed embeddings': (_embed_as(lambda v: v.t().contiguous().t()), 'converted'),
    'row-strided embeddings': (_every_other_row_strided, 'converted'),
    'integer numpy embeddings': (_embed_as(lambda v: (v * 100).round().cpu().numpy().astype(np.int32)), 'converted'),
    'embeddings one row short': (_embed_as(lambda v: v[:-1]), 'converted'),
    'domains given': (lambda fps: [setattr(fp, 'domains', ['1-20', '5-9,30-40']) for fp in fps[::3]], 'converted'),
    'mixed plain and converted': (_mixed, 'converted'),
    'cuda float16 embeddings': (_embed_as(lambda v: v.half()), 'flush'),
    'cuda bfloat16 embeddings': (_embed_as(lambda v: v.bfloat16()), 'flush'),
}


@pytest.mark.parametrize('kind', list(_INPUT_KINDS) + ['quants present'])
def test_every_input_kind_through_the_one_flush_equals_queue_cpu(kind):
    """What the flush does not take as it is -- numpy / CPU / flat maps, numpy / CPU / integer / transposed / row-strided
    embeddings, embeddings of another length than the sequence, domains given by the caller, fingerprints already there (a
    second flush on the same objects: the reference's second quantize) -- is converted and goes through the same flush, with
    the results of queue_cpu run protein by protein (one protein handed back to the host library inside); the writer's records
    are those of the objects.  Half-precision GPU embeddings are taken as they are."""
    from dctdomain_amd import make_db
    lens = [120, 31, 260, 45, 2100, 330, 700, 97, 22, 410, 150, 80]
    fresh = _embedded(lens, seed=17)
    if kind == 'quants present':
        got = make_db.fingerprint_batch(make_db.fingerprint_batch(fresh(), threads=4), threads=4)
        path = make_db.LAST_PATH[0]
        ref = [make_db.queue_cpu(make_db.queue_cpu(fp)) for fp in fresh()]
        recs = make_db.flush_records(make_db.fingerprint_batch(fresh(), threads=4), threads=4)
        want = 'converted'
    else:
        change, want = _INPUT_KINDS[kind]
        fps, ref, more = fresh(), fresh(), fresh()
        for x in (fps, ref, more):
            change(x)
        got = make_db.fingerprint_batch(fps, threads=4)
        path = make_db.LAST_PATH[0]
        ref = [make_db.queue_cpu(fp) for fp in ref]
        recs = make_db.flush_records(more, threads=4)
    assert path == want and make_db.LAST_PATH[0] == want, (kind, path, make_db.LAST_PATH[0])
    _assert_same_as_queue_cpu(got, ref)
    assert sum(len(fp.domains) > 1 for fp in ref) >= 3
    for r, e in zip(recs, make_db._records(ref)):
        assert r[0] == e[0] and r[1] == e[1]
        assert r[2].dtype == np.int8
        np.testing.assert_array_equal(r[2], e[2])


def test_inputs_the_flush_refuses_raise_what_they_raised():
    """Embeddings far shorter than their sequences (a domain of 2 rows: the reference's reshape fails) and float32 and float64
    proteins in one layer raise ValueError, as they did before the flush took every input; the next flush is whole."""
    from dctdomain_amd import make_db
    fresh = _embedded([120, 260, 45, 330], seed=19)
    for fn in (make_db.fingerprint_batch, make_db.flush_records):
        fps = fresh()
        for fp in fps:
            fp.embed = {k: v[:2] for k, v in fp.embed.items()}
        with pytest.raises(ValueError):
            fn(fps, threads=2)
        fps = fresh()
        for fp in fps[1::2]:
            fp.embed = {k: v.double() if k == 15 else v for k, v in fp.embed.items()}
        with pytest.raises(ValueError):
            fn(fps, threads=2)
    recs, ref = make_db.flush_records(fresh(), threads=2), [make_db.queue_cpu(fp) for fp in fresh()]
    assert make_db.LAST_PATH[0] == 'flush'
    for r, e in zip(recs, make_db._records(ref)):
        assert r[1] == e[1]
        np.testing.assert_array_equal(r[2], e[2])


def test_process_sequences_with_deferred_second_halves_keeps_the_order():
    """process_sequences finishes a flush when the next one has been started: the records must reach the writer in sequence order
    and equal those of one big flush."""
    from dctdomain_amd import make_db
    from dctdomain_amd.embedding import SyntheticModel
    rng = np.random.default_rng(9)
    aa = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)
    seqs = [(f's{i:03d}', aa[rng.integers(0, 20, size=int(L))].tobytes().decode())
            for i, L in enumerate(np.clip(rng.gamma(2.0, 120.0, size=90).astype(int), 25, 900))]
    dev = torch.device('cuda', 0)
    model = SyntheticModel()
    model.to_device(dev)

    def run(flush):
        got, sizes = [], []
        make_db.process_sequences(seqs, model, dev, 500, 4, flush, lambda recs: (got.extend(recs), sizes.append(len(recs))))
        return got, sizes
    small, sizes = run(16)
    big, one = run(10 ** 6)
    assert len(sizes) >= 4 and len(one) == 1 and [r[0] for r in small] == [p for p, _ in seqs] == [r[0] for r in big]
    for x, y in zip(small, big):
        assert x[1] == y[1]
        np.testing.assert_array_equal(x[2], y[2])


def test_cutter_in_flight_while_the_callers_stream_uses_the_context():
    """The first half of a flush leaves its contact selection and cutter running on a side stream; the caller's stream goes on using
    the SAME context -- window stitching (job tables in the context's double-buffered table block), another domain prediction
    (the cutter's adjacency scratch), a fingerprint call.  Every one of them must queue behind the readers of what it overwrites
    (a build once did not: stitch_impl uploaded its table over the cutter's) -- the flush's results must be
    those of the flush run alone."""
    from dctdomain_amd import make_db, reccut
    from dctdomain_amd.embedding import stitch_embeddings_batch, stitch_contacts_batch
    rng = np.random.default_rng(12)
    lens = np.clip(rng.gamma(2.2, 170.0, size=700).astype(int), 60, 1300).tolist()
    fresh = _embedded(lens, seed=8)
    alone = make_db.flush_records(fresh(), threads=4)
    dev = torch.device('cuda', 0)
    wins = [[torch.randn(500, 640, device=dev), torch.randn(350, 640, device=dev)] for _ in range(3)]
    cwins = [[torch.rand(500, 500, device=dev), torch.rand(400, 400, device=dev)]]
    other = [fp.contacts for fp in fresh()[:40]]
    other_alone = reccut.domains_from_maps(other, 2.6)
    for rep in range(3):
        fl = make_db._Flush(fresh(), threads=4)
        assert fl.start()
        # ... the caller's stream, while the cutter runs: both table buffers several times over, the cutter's scratch, a quantize
        for _ in range(4):
            stitch_embeddings_batch(wins)
            stitch_contacts_batch(cwins, 300)
        assert reccut.domains_from_maps(other, 2.6) == other_alone
        few = make_db.flush_records(fresh()[:8], threads=2)
        recs = fl.finish(objects=False)
        assert recs is not None and len(recs) == len(alone)
        for a, b in zip(alone, recs):
            assert a[0] == b[0] and a[1] == b[1]
            np.testing.assert_array_equal(a[2], b[2])
        for a, b in zip(alone[:8], few):
            assert a[1] == b[1]
            np.testing.assert_array_equal(a[2], b[2])


def test_three_flushes_in_flight_finished_out_of_order():
    """A flush owns its page-locked result buffers from start() to the end of finish(): three flushes started before the first is
    finished, finished out of order, each give what flush_records gives for their proteins alone (with two sets of buffers shared
    by turns, the third start() wrote over the first flush's results, and its finish() decoded them without an error)."""
    from dctdomain_amd import make_db
    rng = np.random.default_rng(21)
    lens = np.clip(rng.gamma(2.2, 160.0, size=360).astype(int), 40, 1300).tolist()
    fresh = _embedded(lens, seed=11)
    groups = [slice(0, 90), slice(90, 220), slice(220, 360)]
    alone = [make_db.flush_records(fresh()[g], threads=4) for g in groups]
    flushes = [make_db._Flush(fresh()[g], threads=4) for g in groups]
    for fl in flushes:
        assert fl.start()
    for i in (1, 2, 0):
        recs = flushes[i].finish(objects=False)
        assert recs is not None and len(recs) == len(alone[i])
        for a, b in zip(alone[i], recs):
            assert a[0] == b[0] and a[1] == b[1]
            np.testing.assert_array_equal(a[2], b[2])


def test_flush_on_padded_batches_every_protein_against_the_oracles():
    """Batches of several sequences through Batch.embed_parallel: every protein's contact map is a view of the batch's padded
    (B, W, W) tensor, row stride W, W of every residue mod 4, member lengths of every residue mod 4 (16-byte loads whose last
    one crosses the end of a row, maps 4 bytes off a 16-byte boundary), plus one protein longer than 2 048 alone in its batch
    (handed back to the host library).  The flush must take them all, and EVERY protein must get the host library's cut of the
    oracle's top contacts on its contiguous map (and the reference binary's strings, where it is built) and the oracle's quants."""
    import dctdomain_amd as dd
    from dctdomain_amd import make_db, reccut
    from dctdomain_amd.embedding import Batch, SyntheticModel
    from oracle import contacts_oracle as co
    from oracle import dct_oracle as orc
    rng = np.random.default_rng(404)
    aa = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)
    dev = torch.device('cuda', 0)
    model = SyntheticModel(dim=640)
    model.to_device(dev)
    embeds, widths = [], []
    for W in (440, 361, 282, 203, 2101):
        lens = [W] if W > 2048 else [W] + [int(rng.integers(30, W - 3)) // 4 * 4 + r for r in (0, 1, 2, 3, 3, 2, 1, 0)]
        b = Batch([(f'w{W}_{q}', aa[rng.integers(0, 20, size=L)].tobytes().decode()) for q, L in enumerate(lens)], model, dev)
        b.embed_parallel([15, 21])
        for e in b.embeds:
            assert e.contacts.shape == (len(e.seq), len(e.seq))
            assert len(e.seq) < 2 or e.contacts.stride(0) == W
        embeds += b.embeds
        widths += [W] * len(b.embeds)
    lens = [len(e.seq) for e in embeds]
    assert {W % 4 for W in widths} == {0, 1, 2, 3}
    for W in set(widths) - {2101}:
        assert {L % 4 for L, w in zip(lens, widths) if w == W and L < W} == {0, 1, 2, 3}
    assert any(e.contacts.data_ptr() % 16 for e in embeds)
    fps = [dd.Fingerprint(pid=e.pid, seq=e.seq, embed=e.embed, contacts=e.contacts) for e in embeds]
    make_db.fingerprint_batch(fps, threads=4)
    assert make_db.LAST_PATH[0] == 'flush'
    assert reccut.LAST.host_redo == [lens.index(2101)]
    have_ref = os.path.exists(co.REF_BIN)
    n_multi = 0
    for e, fp, L in zip(embeds, fps, lens):
        cmap = e.contacts.contiguous().cpu().numpy()
        ci, cj, cv = co.top_contacts(cmap, 2.6)
        d = reccut.domains_from_contacts([L], [0, len(ci)], ci, cj, cv)[0]
        exp = d + [f'1-{L}'] if len(d) > 1 else d
        assert fp.domains == exp, (fp.pid, L, fp.domains, exp)
        if have_ref:
            rc, out = co.run_ref_binary(co.ce_text(fp.pid, fp.seq, ci, cj, cv))
            assert rc == 0 and co.parse_reccut(out, L) == exp, (fp.pid, L)
        q = orc.quantize([e.embed[15].cpu().numpy(), e.embed[21].cpu().numpy()], exp, [3, 80, 3, 80])
        assert list(fp.quants) == list(q) == exp
        for k in q:
            np.testing.assert_array_equal(fp.quants[k], q[k], err_msg=f'{fp.pid} {k}')
        n_multi += len(exp) > 1
    assert n_multi >= 5
