"""Host-side data path: tokenizer against goldens produced by the reference's tokenizer
(tools/make_golden_tokenizer.py), the frame-folder dataset on a synthetic folder, the gif / png writers."""
import json
import os

import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def vocab(tmp_path_factory):
    """The reference's CLIP merge table as SimpleTokenizer reads it (header + the 48,894 merges it uses), unpacked from
    tests/golden/bpe_merges.txt.xz (tools/make_golden_tokenizer.py)."""
    import lzma
    path = tmp_path_factory.mktemp('bpe') / 'bpe_simple_vocab_16e6.txt'
    with lzma.open(os.path.join(GOLDEN, 'bpe_merges.txt.xz'), 'rb') as src:
        path.write_bytes(src.read())
    return str(path)


def test_tokenizer_matches_reference_goldens(vocab):
    from mmvid_amd.data import SimpleTokenizer
    g = json.load(open(os.path.join(GOLDEN, 'tokenizer.json')))
    tok = SimpleTokenizer(vocab)
    assert tok.vocab_size == g['vocab_size'] == 49408 and len(tok.encoder) == 49408
    for r in g['rows']:
        ids = tok.encode(r['text'])
        assert ids == r['ids'], r['text']
        assert tok.decode(ids) == r['decoded'] and tok.decode(ids, remove_start_end=False) == r['decoded_keep']
    texts = [r['text'] for r in g['rows']]
    assert tok.tokenize(texts[:4], context_length=64).tolist() == g['tokenize_64']
    assert tok.tokenize([texts[8]], context_length=8, truncate_text=True).tolist() == g['truncate_8']
    with pytest.raises(RuntimeError, match='too long'):
        tok.tokenize([texts[8]], context_length=8)
    assert tok.decode(torch.tensor([49406, 320, 0, 0])) == tok.decode([320])  # start token and padding are dropped


def test_tokenizer_without_the_merge_table_fails_loudly(tmp_path, monkeypatch):
    from mmvid_amd.data import SimpleTokenizer
    monkeypatch.delenv('MMVID_BPE_VOCAB', raising=False)
    with pytest.raises(FileNotFoundError, match='merge table'):
        SimpleTokenizer(str(tmp_path / 'missing.txt'))


class _FakeTok:
    def tokenize(self, text, n, truncate_text=False):
        ids = [ord(c) % 251 + 1 for c in text][:n]
        out = torch.zeros(1, n, dtype=torch.long)
        out[0, :len(ids)] = torch.tensor(ids)
        return out


def _make_folder(root, lengths):
    import numpy as np
    from PIL import Image
    for key, n in lengths.items():
        os.makedirs(root / 'video' / key)
        for i in range(n):
            arr = np.full((40, 56, 3), (i * 9) % 256, np.uint8)
            arr[:, :, 1] = (len(key) * 31) % 256
            Image.fromarray(arr).save(root / 'video' / key / f'frame{i}.png')
    os.makedirs(root / 'txt')
    for key in list(lengths)[:-1]:  # the last video has no caption -> it is not part of the dataset
        (root / 'txt' / f'{key}.txt').write_text(f'caption of {key}\nsecond line ignored')


def test_text_video_dataset_layout_and_sampling(tmp_path):
    from mmvid_amd.data import TextVideoDataset
    _make_folder(tmp_path, {'clip_b': 20, 'clip_a': 12, 'short': 5, 'uncaptioned': 30})
    ds = TextVideoDataset(tmp_path, text_len=16, image_size=32, tokenizer=_FakeTok(), frame_step=2, frame_num=4, deterministic=True)
    assert ds.keys == ['clip_a', 'clip_b'] and ds.min_len == 8  # 'short' < max(8, 3*2+1) frames, 'uncaptioned' has no txt
    tokens, frames, visual = ds[1]  # the reference's contract (loader.py:500-562): `text, frames, visuals = batch`
    assert tokens.shape == (16, ) and tokens[0] == ord('c') % 251 + 1
    assert visual.shape == (3, 32, 32) and torch.equal(visual, frames[0])  # deterministic: frame 0 of the video
    assert frames.shape == (4, 3, 32, 32) and 0.0 <= float(frames.min()) and float(frames.max()) <= 1.0
    # natural order (frame10 after frame9) and a stride of two frames from frame 0: grey levels 0, 18, 36, 54
    assert [round(float(f[0, 0, 0]) * 255) for f in frames] == [0, 18, 36, 54]
    # the training transform: random start + one random-resized square crop for all frames, reproducible from a generator
    mk = lambda s: TextVideoDataset(tmp_path, text_len=16, image_size=32, tokenizer=_FakeTok(), frame_step=2, frame_num=4,
                                    generator=torch.Generator().manual_seed(s))
    a, b, c = mk(3)[1][1], mk(3)[1][1], mk(4)[1][1]
    assert torch.equal(a, b) and a.shape == (4, 3, 32, 32)
    starts = {round(float(mk(s)[1][1][0, 0, 0, 0]) * 255) // 9 for s in range(12)}
    assert len(starts) > 1 and max(starts) <= 20 - 6 - 1  # start in [0, len - span - 1], as random.randint's inclusive bound
    # video_only keeps the (text, frames, visual) order with the reference's 'dummy text' placeholder
    vo = TextVideoDataset(tmp_path, text_len=16, image_size=32, tokenizer=_FakeTok(), frame_num=4, video_only=True, deterministic=True)[0]
    assert len(vo) == 3 and vo[0].shape == (16, ) and vo[0][0] == ord('d') % 251 + 1 and vo[1].shape == (4, 3, 32, 32)
    # a random non-empty caption line when not deterministic
    (tmp_path / 'txt' / 'clip_b.txt').write_text('caption one\n\nzebra two\n')
    firsts = {int(mk(s)[1][0][0]) for s in range(16)}
    assert firsts == {ord('c') % 251 + 1, ord('z') % 251 + 1}


def test_save_image_tensor_gif_and_png(tmp_path):
    from PIL import Image

    from mmvid_amd.data import save_image_tensor
    video = torch.rand(1, 5, 3, 16, 24) * 1.4 - 0.2  # values outside [0, 1] are clamped
    name = save_image_tensor(video, tmp_path / 'sample')
    assert name == 'sample.gif'
    with Image.open(tmp_path / name) as im:
        assert im.n_frames == 5 and im.size == (24, 16)
    img = torch.linspace(0, 1, 3 * 8 * 8).view(3, 8, 8)
    assert save_image_tensor(img, tmp_path / 'still') == 'still.png'
    with Image.open(tmp_path / 'still.png') as im:
        import numpy as np
        px = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1)
    assert torch.equal(px, (img * 255).to(torch.uint8))  # truncation, as `(x * 255).type(torch.uint8)` in the reference


def _boxes(buf, start=0, end=None):
    """[(type, payload offset, payload size)] of the ISO base-media boxes in buf[start:end]."""
    out, pos, end = [], start, len(buf) if end is None else end
    while pos < end:
        size, kind = int.from_bytes(buf[pos:pos + 4], 'big'), buf[pos + 4:pos + 8].decode('latin1')
        assert size >= 8 and pos + size <= end, (kind, size)
        out.append((kind, pos + 8, size - 8))
        pos += size
    return out


def test_save_image_tensor_mp4_is_motion_jpeg_in_iso_bmff(tmp_path):
    """utils_html.py:178-184 (`video_format='mp4'`, 4 fps): the file is parsed back box by box -- ftyp / mdat / moov, one video
    track whose sample table (stts / stsc / stsz / stco) locates every frame -- and each sample decodes (PIL) to the frame written,
    within JPEG quality-95 error."""
    import io

    import numpy as np
    from PIL import Image

    from mmvid_amd.data import save_image_tensor
    torch.manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 32), torch.linspace(0, 1, 48), indexing='ij')
    video = torch.stack([torch.stack([(xx + 0.1 * t) % 1.0, yy, 0.5 * (xx + yy)]) for t in range(6)])  # smooth content [6,3,32,48]
    assert save_image_tensor(video.unsqueeze(0), tmp_path / 'clip', video_format='mp4') == 'clip.mp4'
    buf = (tmp_path / 'clip.mp4').read_bytes()
    top = {k: (o, n) for k, o, n in _boxes(buf)}
    assert list(top) == ['ftyp', 'mdat', 'moov'] and buf[top['ftyp'][0]:top['ftyp'][0] + 4] == b'isom'
    moov = {k: (o, n) for k, o, n in _boxes(buf, top['moov'][0], sum(top['moov']))}
    o, n = moov['mvhd']
    scale, duration = int.from_bytes(buf[o + 12:o + 16], 'big'), int.from_bytes(buf[o + 16:o + 20], 'big')
    assert duration / scale == 6 / 4  # six frames at four per second
    trak = {k: (o, n) for k, o, n in _boxes(buf, moov['trak'][0], sum(moov['trak']))}
    o, n = trak['tkhd']
    assert int.from_bytes(buf[o + 76:o + 80], 'big') >> 16 == 48 and int.from_bytes(buf[o + 80:o + 84], 'big') >> 16 == 32
    mdia = {k: (o, n) for k, o, n in _boxes(buf, trak['mdia'][0], sum(trak['mdia']))}
    assert buf[mdia['hdlr'][0] + 8:mdia['hdlr'][0] + 12] == b'vide'
    minf = {k: (o, n) for k, o, n in _boxes(buf, mdia['minf'][0], sum(mdia['minf']))}
    stbl = {k: (o, n) for k, o, n in _boxes(buf, minf['stbl'][0], sum(minf['stbl']))}
    o, n = stbl['stsd']
    assert buf[o + 12:o + 16] == b'jpeg' and int.from_bytes(buf[o + 40:o + 42], 'big') == 48 and int.from_bytes(buf[o + 42:o + 44], 'big') == 32
    o, n = stbl['stts']
    assert [int.from_bytes(buf[o + 4 * i:o + 4 * i + 4], 'big') for i in range(1, 4)] == [1, 6, scale // 4]
    o, n = stbl['stsz']
    sizes = [int.from_bytes(buf[o + 12 + 4 * i:o + 16 + 4 * i], 'big') for i in range(int.from_bytes(buf[o + 8:o + 12], 'big'))]
    o, n = stbl['stco']
    pos = int.from_bytes(buf[o + 8:o + 12], 'big')
    assert len(sizes) == 6 and pos == top['mdat'][0] and sum(sizes) == top['mdat'][1]
    want = (video.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).numpy().astype(np.int16)
    for t, size in enumerate(sizes):
        with Image.open(io.BytesIO(buf[pos:pos + size])) as im:
            assert im.format == 'JPEG' and im.size == (48, 32)
            got = np.asarray(im.convert('RGB')).astype(np.int16)
        assert np.abs(got - want[t]).mean() < 2.0 and np.abs(got - want[t]).max() < 24
        pos += size


def test_reference_import_paths():
    """utils_train.py:25,187 import these names from `mmvid_pytorch.loader` / `.tokenizer`: the same module paths exist here."""
    from mmvid_amd import data
    from mmvid_amd.loader import TextVideoDataset
    from mmvid_amd.tokenizer import SimpleTokenizer
    assert TextVideoDataset is data.TextVideoDataset and SimpleTokenizer is data.SimpleTokenizer
    from mmvid_amd.loader_ext import VoxDataset  # utils_train.py:17 `from mmvid_pytorch.loader_ext import VoxDataset`
    assert VoxDataset.__init__.__code__.co_varnames[1:22] == (
        'folder', 'text_len', 'image_size', 'truncate_captions', 'resize_ratio', 'tokenizer', 'shuffle', 'mode', 'frame_step', 'frame_num',
        'deterministic', 'cache', 'return_vc', 'video_only', 'keys', 'return_neg', 'attr_mode', 'sample_label', 'cat1', 'args', 'rng')


# ------------------------------------------------------------------------------------------------ VoxCeleb loader (loader_ext.py)
def _make_vox(root, spec, with_aux=True):
    """spec: {key: (frames, label flags set)} -> video / txt / label / mask / draw trees of mm_vox_celeb/README.md:12-42.  Frame t
    of every video is a flat grey level 9 t, masks are 200, drawings 100."""
    import numpy as np
    from PIL import Image
    for key, (nframes, flags) in spec.items():
        for sub, level in (('video', None), ('mask', 200), (os.path.join('draw', 'style1'), 100)):
            if sub != 'video' and not with_aux:
                continue
            d = root / sub / key
            d.mkdir(parents=True, exist_ok=True)
            for t in range(nframes if sub == 'video' else 3):
                v = min(9 * t, 255) if level is None else level
                Image.fromarray(np.full((40, 56, 3), v, np.uint8)).save(d / f'{t:07d}.png')
        (root / 'txt').mkdir(exist_ok=True)
        (root / 'label').mkdir(exist_ok=True)
        (root / 'txt' / f'{key}.txt').write_text(f'{key[:4]} talks.\n\nzz second line.\n')
        (root / 'label' / f'{key}.txt').write_text(','.join('1' if i in flags else '0' for i in range(40)))


VOX = {'id01#aaa#0001.txt#000.mp4': (20, {20, 39}), 'id01#aaa#0002.txt#000.mp4': (12, {20}), 'id02#bbb#0001.txt#000.mp4': (16, {4, 15, 39}),
       'id03#ccc#0001.txt#000.mp4': (5, {13})}


def test_vox_dataset_index_caches_and_contract(tmp_path):
    """loader_ext.py:143-311: the index (and its two pickle caches, in the reference's format), the short-video filter, the person /
    attribute tables, and the (text, frames, visuals) contract in the default attr_mode."""
    import pickle

    from mmvid_amd.loader_ext import VoxDataset, person_id
    root = tmp_path / 'mmvox'
    root.mkdir()
    _make_vox(root, VOX)
    ds = VoxDataset(root, text_len=16, image_size=32, tokenizer=_FakeTok(), frame_step=2, frame_num=4, deterministic=True, attr_mode='mask+text')
    assert sorted(ds.keys) == sorted(k for k, (n, _) in VOX.items() if n >= 8) and ds.min_len == 8
    idx = pickle.load(open(tmp_path / 'mmvox_local.pkl', 'rb'))
    assert set(idx) == {'root', 'keys', 'texts', 'videos', 'lengths'} and len(idx['keys']) == 4  # the cache holds every video
    k0 = 'id01#aaa#0001.txt#000.mp4'
    assert idx['texts'][k0] == os.path.join('txt', k0 + '.txt') and idx['videos'][k0][10] == os.path.join('video', k0, '0000010.png')
    attr = pickle.load(open(tmp_path / 'mmvox_attr_dict_vox2.pkl', 'rb'))
    assert set(attr) == {'pid', 'attr', 'cat1'} and sorted(attr['pid']['id01#aaa']) == sorted(k for k in VOX if k.startswith('id01'))
    assert person_id(k0) == 'id01#aaa' and sorted(ds.attr_dict['cat1'][39]) == sorted([k0, 'id02#bbb#0001.txt#000.mp4'])
    assert ds.attr_dict['cat1'][13] == []  # its only holder is the 5-frame video, filtered out
    i = ds.keys.index(k0)
    tokens, frames, visuals = ds[i]
    assert tokens.shape == (16, ) and tokens[0] == ord('i') % 251 + 1  # deterministic: the first caption line
    assert frames.shape == (4, 3, 32, 32) and [round(float(f[0, 0, 0]) * 255) for f in frames] == [0, 18, 36, 54]
    assert visuals.shape == (1, 3, 32, 32) and round(float(visuals[0, 0, 5, 5]) * 255) == 200  # the mask frame
    # a second instance reads both caches instead of scanning (the folder can even be gone)
    import shutil
    shutil.rmtree(root / 'txt')
    again = VoxDataset(root, text_len=16, image_size=32, tokenizer=_FakeTok(), frame_step=2, frame_num=4, deterministic=True, video_only=True)
    assert sorted(again.keys) == sorted(ds.keys)
    tok, fr, vis = again[0]
    assert tok[0] == ord('d') % 251 + 1 and fr.shape == (4, 3, 32, 32) and vis.shape == (3, 32, 32)  # 'dummy text', own frame 0


def test_vox_dataset_attr_modes(tmp_path):
    """The control images and captions of every attr_mode (loader_ext.py:470-787): sources by their grey level (video frames < 180,
    masks 200, drawings 100), the two-image sentences name what sits in which slot, dropout yields 'null', cat1 / cat2 return stacks."""
    import random

    from mmvid_amd.loader_ext import _RECIPES, VoxDataset
    root = tmp_path / 'mmvox'
    root.mkdir()
    _make_vox(root, VOX)

    def level(img):
        return round(float(img[0, 4, 4]) * 255)

    def kind(img):
        return {200: 'mask', 100: 'draw'}.get(level(img), 'appearance')

    for mode, recipe in _RECIPES.items():
        seen = set()
        for seed in range(24):
            ds = VoxDataset(root, text_len=96, image_size=32, tokenizer=None, frame_step=2, frame_num=4, attr_mode=mode, rng=random.Random(seed))
            text, frames, visuals = ds[seed % len(ds)]
            assert frames.shape == (4, 3, 32, 32) and visuals.dim() == 4 and visuals.shape[1:] == (3, 32, 32)
            if recipe['caption'] == 'pair':
                assert visuals.shape[0] == 2
                a, b = kind(visuals[0]), kind(visuals[1])
                assert text in (f'A person with {a} in image one and {b} in image two is talking',
                                f'A person with {b} in image two and {a} in image one is talking'), (mode, text)
                seen.add((a, b, text.startswith(f'A person with {a}')))
            elif recipe['caption'] == 'one':
                assert text == 'A person in image one is talking' and kind(visuals[0]) == mode
            elif recipe['caption'] == 'motion':
                assert visuals.shape[0] == 1 + len(frames[:9:3]) and text.endswith('motion in the following frames is talking.')
                assert torch.equal(visuals[1:], frames[:9:3])  # every third frame of the clip (3 of them with the usual 8-frame clips)
            else:
                assert text in ('null', 'id01 talks.', 'id02 talks.', 'zz second line.')
                seen.add(text)
        if recipe['caption'] == 'pair':
            orders = {s[:2] for s in seen}
            assert len(orders) == (2 if recipe.get('shuffle') else 1) and {s[2] for s in seen} == {True, False}, (mode, seen)
    # dropout: about one caption in ten becomes 'null'
    ds = VoxDataset(root, text_len=96, image_size=32, tokenizer=None, frame_step=2, frame_num=4, attr_mode='mask+text_dropout', rng=random.Random(5))
    nulls = sum(ds[i % len(ds)][0] == 'null' for i in range(300))
    assert 10 <= nulls <= 55
    # negative captions: a video with different attribute flags
    ds = VoxDataset(root, text_len=16, image_size=32, tokenizer=_FakeTok(), frame_step=2, frame_num=4, attr_mode='text', return_neg=True,
                    rng=random.Random(1))
    out = ds[0]
    assert len(out) == 5 and out[3] == 0 and out[4].shape == (16, ) and out[2].shape == (1, 3, 32, 32)
    # cat1 / cat2: one clip per attribute with a sentence about it
    ds = VoxDataset(root, text_len=96, image_size=32, tokenizer=None, frame_step=2, frame_num=4, attr_mode='cat1', cat1=[39, 15], rng=random.Random(2))
    clips, texts = ds[0]
    assert clips.shape == (2, 4, 3, 32, 32) and texts == ['A person is young.', texts[1]] and texts[1] in ('A person wears eyeglasses.', 'A person is wearing eyeglasses.')
    ds = VoxDataset(root, text_len=96, image_size=32, tokenizer=None, frame_step=2, frame_num=4, attr_mode='cat2', rng=random.Random(2))
    with pytest.raises((KeyError, ZeroDivisionError)):  # no kept video is chubby: the attribute's list is empty (as in the reference)
        ds[0]
    _make_vox(root, {'id04#ddd#0001.txt#000.mp4': (10, {4, 13, 15, 39})})
    for f in (tmp_path / 'mmvox_local.pkl', tmp_path / 'mmvox_attr_dict_vox2.pkl'):
        f.unlink()
    ds = VoxDataset(root, text_len=96, image_size=32, tokenizer=None, frame_step=2, frame_num=4, attr_mode='cat2', rng=random.Random(2))
    clips, texts = ds[ds.keys.index('id01#aaa#0001.txt#000.mp4')]
    assert clips.shape == (5, 4, 3, 32, 32) and texts[0] in ('A boy.', 'A guy.') and texts[1:] == [
        'A person is youthful.', 'A person has no hair.', 'A person wears spectacles.', 'A person is plump.']


def test_vox_text_grammar():
    """mm_vox_celeb/pcfg.py restated (mmvid_amd/vox_text.py): sentence forms, attribute grouping, negated 'No_' labels, exclusive hair
    colours.  The attribute tables themselves are compared with the reference module's (tests/golden/vox_attr_tables.json,
    tools/make_golden_tokenizer.py)."""
    import random
    import re

    from mmvid_amd import vox_text as vt
    r = random.Random(0)
    forms = re.compile(r"^(He|She|A (male|man|female|woman|person)|This (male|man|female|woman|person)) (is|has|wears|is wearing) [a-z' ,0-9]+\.$")
    for _ in range(200):
        verb = r.choice(['is', 'has', 'wear'])
        s = vt.generate_phrase((r.random() < 0.5, r.random()), (verb, 'wavy hair'), r)
        assert forms.match(s), s
    assert vt.generate_phrase((True, 1.0), ('has', 'bangs'), r) == 'He has bangs.' and vt.generate_phrase((False, 1.0), ('is', 'young'), r) == 'She is young.'
    pred = [False] * 40
    for a in ('Male', 'Young', 'Eyeglasses', 'Wavy_Hair', 'Bangs', 'Big_Nose', 'No_Beard'):
        pred[vt.ATTR.index(a)] = True
    text = vt.generate(pred, 3, r)
    assert len(text) == 3 and all('beard' not in t for t in text)  # No_Beard = 1 means no beard: negated away
    for t in text:
        assert all(forms.match(s + '.') for s in t.rstrip('.').split('. ')), t
        for word in ('young', 'eyeglasses', 'wavy hair', 'bangs', 'big nose'):
            assert t.count(word) == 1
        assert 'She' not in t and 'woman' not in t and 'female' not in t
    pred[vt.ATTR.index('No_Beard')] = False
    assert all('beard' in t for t in vt.generate(pred, 2, r))
    many = [vt.mutual_exclusive([True] * 40, vt.HAIR_COLOURS, r) for _ in range(20)]
    assert all(sum(m[vt.ATTR.index(a)] for a in vt.HAIR_COLOURS) == 1 for m in many)
    sents = vt.generate_random_sentences(8, 12, r)
    assert len(sents) == 12 and all('smiling' not in s and 'blurry' not in s and 'brown hair' not in s for s in sents)
    ref = json.load(open(os.path.join(GOLDEN, 'vox_attr_tables.json')))
    assert ref['ATTR'] == vt.ATTR and ref['NAME'] == list(vt.NAME) and ref['ATTR_VERB'] == vt.ATTR_VERB
    assert ref['NEGATE_IDX'] == vt.NEGATE_IDX and ref['GENDER_IDX'] == vt.GENDER_IDX


# ------------------------------------------------------------------------------------------------ one file per video (loader.py)
def _make_stacks(root, lengths, vertical=()):
    """video/<id>.png = n square frames of side 24 side by side (or stacked), frame t a flat grey 10 t; txt, label, visual beside."""
    import numpy as np
    from PIL import Image
    for sub in ('video', 'txt', 'label', 'visual'):
        (root / sub).mkdir(parents=True, exist_ok=True)
    for vid, n in lengths.items():
        strip = np.concatenate([np.full((24, 24, 3), min(10 * t, 255), np.uint8) for t in range(n)], axis=0 if vid in vertical else 1)
        Image.fromarray(strip).save(root / 'video' / f'{vid}.png')
        Image.fromarray(255 - strip).save(root / 'visual' / f'{vid}.png')
        (root / 'txt' / f'{vid}.txt').write_text(f'{vid} caption\n')
        (root / 'label' / f'{vid}.txt').write_text('0,1,1,0')


def test_text_image_stack_dataset(tmp_path):
    """loader.py:852-1110: frames split out of one image (horizontal or vertical strip), the index cache, the length filter and the
    four return forms."""
    import pickle
    import random

    import numpy as np

    from mmvid_amd.loader import TextImageStackDataset
    root = tmp_path / 'stacks'
    _make_stacks(root, {'wide': 16, 'tall': 12, 'tiny': 4}, vertical=('tall', ))
    (root / 'video' / 'stray.txt').write_text('not an image')
    ds = TextImageStackDataset(root, text_len=12, image_size=16, tokenizer=_FakeTok(), frame_step=2, frame_num=4, deterministic=True,
                               rng=random.Random(0))
    assert sorted(ds.keys) == ['tall', 'wide'] and ds.lengths == {'wide': 16, 'tall': 12} and ds.has_label and ds.has_visual
    idx = pickle.load(open(tmp_path / 'stacks_local.pkl', 'rb'))
    assert sorted(idx['keys']) == ['tall', 'tiny', 'wide'] and idx['videos']['wide'] == os.path.join('video', 'wide.png')
    for key in ('wide', 'tall'):
        tokens, frames = ds[ds.keys.index(key)]
        assert tokens.shape == (12, ) and tokens[0] == ord(key[0]) % 251 + 1 and frames.shape == (4, 3, 16, 16)
        levels = [round(float(f[0, 3, 3]) * 255) for f in frames]
        assert all(b - a == 20 for a, b in zip(levels, levels[1:])) and levels[0] % 10 == 0  # every second frame of the strip
    vc = TextImageStackDataset(root, text_len=12, image_size=16, tokenizer=_FakeTok(), frame_num=4, deterministic=True, return_vc=True,
                               rng=random.Random(1))
    tokens, frames, visual = vc[0]
    assert visual.shape == (3, 16, 16) and round(float(visual[0, 2, 2]) * 255) % 10 == 5  # 255 - 10 t: a frame of visual/<id>.png
    lab = TextImageStackDataset(root, text_len=12, image_size=16, tokenizer=_FakeTok(), frame_num=4, return_label=True, rng=random.Random(2))[0]
    assert isinstance(lab[2], np.ndarray) and lab[2].tolist() == [0, 1, 1, 0]
    txt = TextImageStackDataset(root, text_len=12, image_size=16, tokenizer=None, frame_num=4, return_text=True, rng=random.Random(2))[1]
    assert txt[0] == txt[2] and txt[2].endswith(' caption')
    img = TextImageStackDataset(root, text_len=12, image_size=16, tokenizer=None, frame_num=4, image_only=True, mode='1frame',
                                rng=random.Random(3))[0]
    assert img[1] == 0 and img[0].shape == (3, 16, 16)
    # no_cache: nothing is written
    (tmp_path / 'stacks_local.pkl').unlink()
    TextImageStackDataset(root, text_len=12, image_size=16, tokenizer=None, frame_num=4, no_cache=True)
    assert not (tmp_path / 'stacks_local.pkl').exists()


def test_text_mp4_dataset_with_an_injected_frame_source(tmp_path):
    """loader.py:597-849 without a decoder: the class takes any source with count(path) / read(path, idxs); without decord and
    without one it says what is missing."""
    import random

    from mmvid_amd.loader import TextMP4Dataset
    from mmvid_amd.loader_files import VID_EXT

    class FakeSource:
        extensions = VID_EXT

        def count(self, path):
            return int(open(path).read())

        def read(self, path, idxs=None):
            n = self.count(path)
            idxs = list(range(n)) if idxs is None else list(idxs)
            return torch.stack([torch.full((3, 20, 28), t / 100.0) for t in idxs])

    root = tmp_path / 'clips'
    for sub in ('video', 'txt', 'label'):
        (root / sub).mkdir(parents=True)
    for vid, n in (('a', 30), ('b', 9), ('c', 5)):
        (root / 'video' / f'{vid}.mp4').write_text(str(n))
        (root / 'txt' / f'{vid}.txt').write_text(f'{vid} words\n')
        (root / 'label' / f'{vid}.txt').write_text('7')
    ds = TextMP4Dataset(root, text_len=10, image_size=16, tokenizer=_FakeTok(), frame_step=2, frame_num=4, source=FakeSource(), rng=random.Random(0))
    assert sorted(ds.keys) == ['a', 'b'] and (tmp_path / 'clips_local.pkl').exists()
    tokens, frames, visual = ds[ds.keys.index('a')]
    assert tokens.shape == (10, ) and frames.shape == (4, 3, 16, 16) and visual.shape == (3, 16, 16)
    t = [round(float(f[0, 0, 0]) * 100) for f in frames]
    assert t == [t[0], t[0] + 2, t[0] + 4, t[0] + 6] and 0 <= t[0] <= 30 - 6 - 1
    assert TextMP4Dataset(root, text_len=10, image_size=16, tokenizer=_FakeTok(), frame_num=4, source=FakeSource(), return_label=True,
                          rng=random.Random(1))[0][2] == 7
    vo = TextMP4Dataset(root, text_len=10, image_size=16, tokenizer=_FakeTok(), frame_num=4, source=FakeSource(), video_only=True, mode='1frame',
                        rng=random.Random(1))[0]
    assert vo[0][0] == ord('d') % 251 + 1 and vo[1].shape == (3, 16, 16) and vo[2].shape == (3, 16, 16)
    try:
        import decord  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='decord'):
            TextMP4Dataset(root, tokenizer=_FakeTok())
