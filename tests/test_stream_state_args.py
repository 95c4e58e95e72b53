"""args.stream_state (--stream_state on the train parser): QMIX in the continuous rollout is opt-in, off by default."""
from marl_dmfb_amd.common.arguments import get_train_args, make_args


def test_stream_state_defaults_off():
    assert get_train_args([]).stream_state is False
    assert get_train_args(['dmfb', '--alg', 'qmix', '-d', '4']).stream_state is False
    assert make_args().stream_state is False


def test_stream_state_parses():
    a = get_train_args(['dmfb', '--alg', 'qmix', '-d', '4', '--stream_state'])
    assert a.stream_state is True and a.alg == 'qmix'
    assert make_args(alg='qmix', stream_state=True).stream_state is True
