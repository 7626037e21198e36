"""hyperreel_amd.data.load_images without a GPU: it tells PNG from JPEG by each file's first bytes, hands the whole list to png.load_png or
jpeg.load_jpeg, and refuses a mixed list, a file that is neither, and an empty list by name.  tests/test_gpu_jpeg_decode.py runs it on
real lists on the device."""
import numpy as np
import pytest

import jpeg_decode_common as D


@pytest.fixture
def files(tmp_path):
    from PIL import Image
    data, want = D.named('w17_h13_420_noise_q95')
    out = {'jpg': [], 'png': []}
    for i in range(2):
        out['jpg'].append(str(tmp_path / f'{i}.jpg'))              # the extension is not what is looked at ...
        with open(out['jpg'][-1], 'wb') as f:
            f.write(data)
        out['png'].append(str(tmp_path / f'{i}.png'))
        Image.fromarray(want['RGB']).save(out['png'][-1])
    out['jpg_named_png'] = str(tmp_path / 'camera.png')              # ... the first bytes are
    with open(out['jpg_named_png'], 'wb') as f:
        f.write(data)
    out['text'] = str(tmp_path / 'poses.txt')
    with open(out['text'], 'w') as f:
        f.write('1 0 0 0\n')
    return out


def test_dispatch_by_signature(files, monkeypatch):
    from hyperreel_amd import data, jpeg, png
    calls = []
    monkeypatch.setattr(png, 'load_png', lambda paths, mode, device: calls.append(('png', list(paths), mode, device)) or 'P')
    monkeypatch.setattr(jpeg, 'load_jpeg', lambda paths, mode, device: calls.append(('jpeg', list(paths), mode, device)) or 'J')
    assert data.load_images(files['png'], 'RGBA') == 'P'
    assert data.load_images(files['jpg'] + [files['jpg_named_png']]) == 'J'
    assert data.load_images(iter(files['jpg']), mode='L', device='cuda:0') == 'J'
    assert calls == [('png', files['png'], 'RGBA', None), ('jpeg', files['jpg'] + [files['jpg_named_png']], 'RGB', None),
                     ('jpeg', files['jpg'], 'L', 'cuda:0')]


def test_refusals_name_the_file(files, monkeypatch):
    from hyperreel_amd import data, jpeg, png
    monkeypatch.setattr(png, 'load_png', lambda *a: pytest.fail('a refused list reached load_png'))
    monkeypatch.setattr(jpeg, 'load_jpeg', lambda *a: pytest.fail('a refused list reached load_jpeg'))
    with pytest.raises(ValueError, match=r'1\.png is a PNG file, .*0\.jpg a JPEG file'):
        data.load_images([files['jpg'][0], files['jpg'][1], files['png'][1]])
    with pytest.raises(ValueError, match=r'camera\.png is a JPEG file'):
        data.load_images([files['png'][0], files['jpg_named_png']])
    with pytest.raises(ValueError, match=r'poses\.txt: neither'):
        data.load_images([files['jpg'][0], files['text']])
    with pytest.raises(ValueError, match='no paths'):
        data.load_images([])


def test_the_jpeg_list_is_what_the_host_build_decodes(files):
    """the files load_images would hand to load_jpeg decode, on the host build, to PIL's pixels"""
    from hyperreel_amd import jpeg
    _, want = D.named('w17_h13_420_noise_q95')
    for p in files['jpg']:
        with open(p, 'rb') as f:
            assert np.array_equal(jpeg.decode_host(f.read(), 'RGB'), want['RGB'])
