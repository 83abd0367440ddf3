"""The launch helper of the ctypes binding (brevitas_amd._native._launch) against a stand-in library, no GPU: the stream
arrives as the entry's last argument, the kernel timer sees the bracket name around the call, and a non-zero return
raises BvqError with the entry's name before the bracket is closed."""
import pytest
import torch

STREAM = 0x5EED


class _Lib:
    """one fake entry and a fake error channel"""

    def __init__(self, rc=0):
        self.rc, self.calls, self.events = rc, [], None

    def bvq_fake(self, *args):
        self.calls.append(args)
        if self.events is not None:
            self.events.append(('call', 'bvq_fake'))
        return self.rc

    def bvq_last_error(self):
        return b'fake: the reason'


class _Timer:
    def __init__(self, events):
        self.events = events

    def before(self, name):
        self.events.append(('before', name))

    def after(self, name):
        self.events.append(('after', name))


@pytest.fixture
def fake(monkeypatch):
    from brevitas_amd import _native as nat
    lib = _Lib()
    lib.events = []
    monkeypatch.setattr(nat, 'lib', lib)
    monkeypatch.setattr(nat, 'stream_ptr', lambda dev: STREAM)
    monkeypatch.setattr(nat, '_timer', None)
    return nat, lib, torch.device('cuda')  # no index: the guard touches no device


def test_the_stream_is_the_last_argument(fake):
    nat, lib, dev = fake
    nat._launch(dev, 'bvq_fake', None, 1, 2.5, None)
    nat._call('bvq_fake', None, 3, 0xABC)  # a wrapper inside `with _DeviceGuard(dev) as stream` passes it itself
    assert lib.calls == [(1, 2.5, None, STREAM), (3, 0xABC)]


def test_the_timer_brackets_the_call_once(fake):
    nat, lib, dev = fake
    nat.set_kernel_timer(_Timer(lib.events))
    nat._launch(dev, 'bvq_fake', 'bvq_other_name', 7)
    assert lib.events == [('before', 'bvq_other_name'), ('call', 'bvq_fake'), ('after', 'bvq_other_name')]


def test_nothing_is_recorded_without_a_bracket_name_or_a_timer(fake):
    nat, lib, dev = fake
    nat._launch(dev, 'bvq_fake', 'bvq_fake', 7)  # no timer set
    nat.set_kernel_timer(_Timer(lib.events))
    nat._launch(dev, 'bvq_fake', None, 7)  # no bracket name
    assert lib.events == [('call', 'bvq_fake')] * 2


def test_a_failing_call_raises_before_the_bracket_closes(fake):
    nat, lib, dev = fake
    lib.rc = -3
    nat.set_kernel_timer(_Timer(lib.events))
    with pytest.raises(nat.BvqError) as e:
        nat._launch(dev, 'bvq_fake', 'bvq_bracket', 7)
    msg = str(e.value)
    assert 'bvq_fake' in msg and '(-3)' in msg and 'fake: the reason' in msg
    assert lib.events == [('before', 'bvq_bracket'), ('call', 'bvq_fake')]
