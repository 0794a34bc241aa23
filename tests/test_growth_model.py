"""The orderings of `lash growth` as the model restates them (growth_model.py): splitmix64's published vectors, one shuffle written
out, and the shuffle being a permutation.  No GPU."""
import growth_model as G


def test_splitmix64_vectors():
    r = G.SplitMix64(1234567)
    assert [r.next(), r.next()] == [6457827717110365317, 3203168211198807973]
    assert G.SplitMix64(0).next() == 0xE220A8397B1DCDAF


# order 1 of ten rows under seed 42, step by step from the rule: state = 42 ^ GAMMA, j = 9 .. 1, r = high word of next() * (j + 1)
def _by_hand(n, state):
    rng, a = G.SplitMix64(state), list(range(n))
    draws = [rng.next() for _ in range(n - 1)]
    for j, z in zip(range(n - 1, 0, -1), draws):
        r = (z * (j + 1)) // (1 << 64)
        a[j], a[r] = a[r], a[j]
    return a


def test_a_shuffle_of_ten_names_written_out():
    names = ["g%d" % i for i in range(10)]
    got = [names[i] for i in G.order(10, 1, 42)]
    assert got == ["g6", "g7", "g4", "g3", "g9", "g5", "g0", "g8", "g2", "g1"]
    assert G.order(10, 1, 42) == _by_hand(10, 42 ^ G.GAMMA)
    assert G.order(10, 0, 42) == list(range(10))                          # order 0 is the rows as they are
    assert G.order(10, 2, 42) != G.order(10, 1, 42) != G.order(10, 1, 43)


def test_the_shuffle_is_a_permutation():
    for n in (1, 2, 1000):
        for o in (1, 2, 7):
            a = G.order(n, o, 42)
            assert sorted(a) == list(range(n)), (n, o)
    assert G.order(1000, 1, 42) != list(range(1000))
    assert G.orders(5, 3, 7).shape == (3, 5) and G.orders(5, 3, 7)[0].tolist() == [0, 1, 2, 3, 4]
