"""The forms maray_lower can emit (include/maray_hip.h, maray_lower_opts), the scenes the lowering-form tests run them on,
and a check that a tape really is the form it is named after -- an option that is silently ignored would otherwise test the
default tape ten times.  Helper module of tests/test_lowering_forms.py (CPU) and tests/test_gpu_lowering_forms.py."""
import maray_amd as M
import tape_eval
from marayb import add, chess, div, encode, max_, min_, mul, nat, sin, step, sub, x, y

# keyword sets of maray_amd.Scene.lower
FORMS = dict(
    default=dict(),
    no_hoist=dict(hoist_rows=False),
    plain_cse=dict(plain_cse=True),
    no_fuse=dict(fuse=False),
    no_skips=dict(skips=False),
    no_row_guards=dict(row_guards=False),
    shared=dict(private_regions=False),
    no_rebalance=dict(rebalance=False),
    no_y_spans=dict(y_spans=False),
    all_off=dict(plain_cse=True, fuse=False, private_regions=False, rebalance=False, y_spans=False),
)

STEPSIN, SIN = tape_eval.OP['STEPSIN'], tape_eval.OP['SIN']


def wave_level_skips(tape):
    """SKIP ops of the PIXEL section that test a value computed per pixel, not a y value: regions a wavefront skips on
    its own lanes' agreement (row_guards=False keeps exactly these)."""
    _, _, pix_ops = tape.arrays()
    n = 0
    for ins in pix_ops:
        op, aux, dst, ra, rb = tape_eval.decode(ins)
        n += op in (tape_eval.OP['SKIPZ'], tape_eval.OP['SKIPNZ']) and ra >> 14 != tape_eval.K_YVAL
    return n


def check_form(name, tape, default_tape):
    """Asserts what makes `tape` the form `name` of the scene whose default lowering is default_tape; returns
    (guards, guards that read Y)."""
    i, d = tape.info, default_tape.info
    n_guards, n_read_y = tape_eval.guards_reading_y(tape)
    d_guards, _ = tape_eval.guards_reading_y(default_tape)
    if name == 'default':
        assert [a.tobytes() for a in tape.arrays()] == [a.tobytes() for a in default_tape.arrays()]
    if name == 'no_hoist':
        assert i['n_row_ops'] == 0 and i['n_yvals'] == 0, (name, i)
    if name == 'no_skips':
        assert i['skip_ops'] == 0 and i['private_regions'] == 0, (name, i)
    if name == 'no_row_guards':
        assert n_guards == 0, (name, n_guards)
        if wave_level_skips(default_tape):           # the default has wave-level regions: they stay
            assert i['skip_ops'] > 0 and wave_level_skips(tape) > 0, (name, i)
    if name in ('shared', 'all_off'):
        assert i['private_regions'] == 0, (name, i)
        if d['skip_ops']:
            assert i['skip_ops'] > 0, (name, i)
    if name in ('no_rebalance', 'all_off') and d['rebalanced_chains']:
        assert i['rebalanced_chains'] == 0, (name, i)
    if name in ('no_fuse', 'all_off') and d['op_histogram'][STEPSIN]:
        assert i['op_histogram'][STEPSIN] == 0 and i['op_histogram'][SIN] > 0, (name, i['op_histogram'])
    if name in ('no_y_spans', 'all_off') and d_guards:
        assert n_read_y > 0, (name, n_guards, n_read_y)
    return n_guards, n_read_y


def lowered_forms(scene):
    """{form: tape} of a maray_amd.Scene, each checked (check_form)."""
    default = scene.lower()
    out = {}
    for name, kw in FORMS.items():
        out[name] = scene.lower(**kw)
        check_form(name, out[name], default)
    return out


def blinds(w, h, n=6):
    """Venetian blinds: n patterns, each behind row bands Step(Sin((y + 7i) / (3 + 2i))), painted over one another.  A band
    has no monotone bound over y, so under the DEFAULT lowering every guard of this scene reads Y (blinds_tape asserts
    it): the specialised back-end falls back to rectangles of one row.  No half-plane or polygon may be added: with a few
    of those the lowering goes back to rectangle guards."""
    from fuzz_scenes import subst_xy
    shapes = []
    for i in range(n):
        band = step(sin(mul(add(y(), nat(7 * i)), div(nat(1), nat(3 + 2 * i)))))
        pattern = subst_xy(chess(2), mul(add(x(), y()), div(nat(1), nat(5 + i))), mul(sub(x(), y()), div(nat(1), nat(7 + i))))
        shapes.append(min_(band, pattern))
    m = shapes[0]
    for s in shapes[1:]:
        m = max_(m, s)
    grad = mul(add(x(), mul(y(), nat(3))), div(nat(1), nat(w + 3 * h)))
    return [mul(m, nat(255)), mul(max_(m, mul(grad, div(nat(1), nat(2)))), nat(255)),
            mul(add(mul(m, div(nat(3), nat(4))), mul(grad, div(nat(1), nat(4)))), nat(255))]


def blinds_tape(scene):
    """The default lowering of a blinds scene (maray_amd.Scene), every guard of which reads Y."""
    tape = scene.lower()
    n_guards, n_read_y = tape_eval.guards_reading_y(tape)
    assert n_read_y == n_guards > 0, (n_guards, n_read_y)
    return tape


def render_with_stale_guards(tape, w, y0, y1, yrows, tile, textures=None):
    """tape_eval.render_with_stale_guards: what a kernel computes that treats a reads-Y tape as rectangle-guarded."""
    return tape_eval.render_with_stale_guards(tape, w, y0, y1, yrows, tile, textures)


# ---- the scenes of the device tests (and of the sensitivity condition) --------------------------------------------------
GPU_SIZE = (320, 96)         # 1.25 tiles of 256 pixels = five 64-pixel runs, the last tile ragged; three 32-row groups


def gpu_scene(name, size=GPU_SIZE):
    """(scene bytes, textures) of the device tests' scenes."""
    import scenes
    from fuzz_scenes import curved_soup, polygon_soup, product_soup
    w, h = size
    if name == 'polygons':       # (fewer shapes where the image is supersampled: the oracle's time at 8 x 8 samples a pixel)
        return encode(size, polygon_soup(2, 24 if size == GPU_SIZE else 8, w, h, mixed=False)), None
    if name == 'curved':
        return encode(size, curved_soup(301, 16, w, h, mixed=True)), None
    if name == 'products':
        return encode(size, product_soup(500, 12, w, h)), None
    if name == 'colours':
        return encode(size, polygon_soup(3, 16, w, h, mixed='colours')), None
    if name == 'blinds':
        return encode(size, blinds(w, h)), None
    assert name == 'guarded_mask'
    return encode(size, scenes.ops_on_a_guarded_mask(w, h)), scenes.textures(scale=64)


SS_SIZE = (160, 48)          # output size of the supersampled device tests (k = 2, 4, 8)
GPU_SCENES = ('polygons', 'curved', 'products', 'colours', 'blinds', 'guarded_mask')


def reads_y_tape(name, size=GPU_SIZE):
    """(scene bytes, tape) of the three tapes whose guards read Y: `blinds` under the default lowering (all guards),
    `polygons` under y_spans=False (all, or nearly), `products` under y_spans=False (the mixed case: some guards read Y,
    some hold for a rectangle)."""
    data, _ = gpu_scene(name, size)
    scene = M.Scene(data)
    if name == 'blinds':
        return data, blinds_tape(scene)
    tape = scene.lower(y_spans=False)
    n_guards, n_read_y = tape_eval.guards_reading_y(tape)
    assert n_read_y > 0 and (n_read_y < n_guards if name == 'products' else 2 * n_read_y > n_guards), (name, n_guards, n_read_y)
    return data, tape


READS_Y = ('blinds', 'polygons', 'products')


def ss_tape(name, k):
    """(supersampled scene, its tape) of one of READS_Y at SS_SIZE output pixels, k x k samples a pixel: the tapes of the
    supersampled device tests.  Guards read Y here too."""
    s = M.Scene(gpu_scene(name, SS_SIZE)[0])
    s.supersample(k)
    tape = blinds_tape(s) if name == 'blinds' else s.lower(y_spans=False)
    n_guards, n_read_y = tape_eval.guards_reading_y(tape)
    assert n_read_y > 0 and (n_read_y < n_guards or name != 'products'), (name, k, n_guards, n_read_y)
    return s, tape
