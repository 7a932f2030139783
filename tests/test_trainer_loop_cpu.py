"""The bookkeeping of Trainer.train (trainer.run_training_loop: epoch roll, validation and save schedule, stop) with counting stubs: no
engine, no GPU."""
import itertools

from hpe_amd.trainer import run_training_loop


class Counter(object):
    def __init__(self):
        self.train, self.val, self.saves, self.lines, self.epochs = [], [], [], [], []

    def train_step(self, gen_batch, critic_batch):
        self.train.append((gen_batch, critic_batch))
        return {"loss": float(len(self.train))}

    def val_step(self, val_batch):
        self.val.append((len(self.train), val_batch))
        return {"loss": 0.0}

    def save(self, epoch):
        self.saves.append((epoch, len(self.train)))

    def summarize(self, epoch, train_results, val_results):
        self.epochs.append((epoch, len(train_results), len(val_results)))
        return "Finished epoch %d" % epoch


def batches():
    return ((("g", i), ("c", i), ("v", i)) for i in itertools.count())


def test_ten_images_batch_four_ten_epochs():
    """num_itr_per_epoch = 10 / 4 = 2.5 is not rounded: the epoch rolls at itr = 3"""
    c = Counter()
    out = run_training_loop(batches(), c.train_step, num_images=10, batch_size=4, max_epoch=10, val_step=c.val_step, validation_step_size=4,
                            save=c.save, summarize=c.summarize, log=c.lines.append)
    assert out == {"steps": 30, "epochs": 10, "saved": [5, 10], "validations": 7}
    assert len(c.train) == 30 and c.train[0] == (("g", 0), ("c", 0)) and c.train[-1] == (("g", 29), ("c", 29))
    assert c.saves == [(5, 15), (10, 30)]  # after epochs 5 and 10, i.e. after 15 and 30 steps
    assert [s for s, _b in c.val] == [4, 8, 12, 16, 20, 24, 28] and c.val[0][1] == ("v", 3)  # the validation batch of that step
    assert [e for e, _t, _v in c.epochs] == list(range(10)) and all(t == 3 for _e, t, _v in c.epochs)
    assert sum(v for _e, _t, v in c.epochs) == 7  # every validation result is summarised in the epoch it fell into
    assert c.lines[0] == "Starting epoch 0" and c.lines[1] == "Finished epoch 0" and c.lines[2].startswith("Starting epoch 1, approx finished in ")
    assert c.lines[-1] == "Finished epoch 9" and sum(l.startswith("Finished") for l in c.lines) == 10


def test_fewer_images_than_a_batch_is_one_step_per_epoch():
    c = Counter()
    out = run_training_loop(batches(), c.train_step, num_images=3, batch_size=8, max_epoch=6, save=c.save, log=c.lines.append)
    assert out == {"steps": 6, "epochs": 6, "saved": [5], "validations": 0}
    assert c.saves == [(5, 5)] and c.lines.count("Finished epoch 4") == 1


def test_exact_multiple_no_validation_without_a_step_size_and_custom_save_interval():
    c = Counter()
    out = run_training_loop(batches(), c.train_step, num_images=8, batch_size=4, max_epoch=3, val_step=c.val_step, validation_step_size=0,
                            save=c.save, save_every=2, log=c.lines.append)
    assert out == {"steps": 6, "epochs": 3, "saved": [2], "validations": 0} and c.val == []


def test_a_finite_source_ends_the_loop_and_zero_epochs_take_no_step():
    c = Counter()
    out = run_training_loop(itertools.islice(batches(), 4), c.train_step, num_images=12, batch_size=4, max_epoch=5, log=c.lines.append)
    assert out["steps"] == 4 and out["epochs"] == 1
    c = Counter()
    out = run_training_loop(batches(), c.train_step, num_images=12, batch_size=4, max_epoch=0, log=c.lines.append)
    assert out["steps"] == 0 and c.train == []
