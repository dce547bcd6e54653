"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

A literal Python 3 restatement of ProbabilityMatrix (SimDataAssessment.py:359-370) and of the matrix part of
MultiStepResolution (SimDataAssessment.py:372-391, "SDA:") of the reference, statement for statement, for
tests/test_connect.py and tests/test_gpu_resolve.py.  It is a same-hand transcription, as the checker of
repeatresolver_amd/window.py is: the script is Python 2 and no Python 2 interpreter was available to run it, so nothing here
is pinned to an execution of the reference.  The only departures: the script's list of resolutions comes with a flank
labelling in front and behind (SDA:375) -- here the caller passes the whole list -- and two labellings give one matrix each
way (the script indexes ForwardMatrices[1] and needs three)."""
import numpy as np


def probability_matrix(Resolution1, Resolution2):
    Resolution1, Resolution2 = [int(x) for x in Resolution1], [int(x) for x in Resolution2]
    Matrix = [[0.0 for t in range(max(Resolution2) + 1)] for tt in range(max(Resolution1) + 1)]                    # SDA:360
    Sums = [len([tt for tt in range(len(Resolution1)) if Resolution1[tt] == t and Resolution2[tt] > -1])
            for t in range(max(Resolution1) + 1)]                                                              # SDA:361
    for t in range(len(Resolution1)):                                                                          # SDA:362-364
        if Resolution1[t] > -1 and Resolution2[t] > -1:
            Matrix[Resolution1[t]][Resolution2[t]] += 1.0
    for t in range(max(Resolution1) + 1):                                                                      # SDA:365-368
        for tt in range(max(Resolution2) + 1):
            if Sums[t] > 0:
                Matrix[t][tt] /= float(Sums[t])
    return np.array(Matrix)                                                                                    # SDA:369


def connection_matrix(AllResolutions):
    """SDA:376-391: AllConCon after the normalisation"""
    ForwardMatrices = []
    BackwardMatrices = []
    for r in range(len(AllResolutions) - 1):                                                                   # SDA:376-378
        ForwardMatrices.append(probability_matrix(AllResolutions[r], AllResolutions[r + 1]))
        BackwardMatrices.append(probability_matrix(AllResolutions[len(AllResolutions) - 1 - r], AllResolutions[len(AllResolutions) - 2 - r]))
    ForwardConCon = ForwardMatrices[0]
    BackwardConCon = BackwardMatrices[0]
    for t in range(1, len(ForwardMatrices)):                                                                   # SDA:379-383
        ForwardConCon = np.dot(ForwardConCon, ForwardMatrices[t])
        BackwardConCon = np.dot(BackwardConCon, BackwardMatrices[t])
    AllConCon = np.multiply(ForwardConCon, np.transpose(BackwardConCon))                                       # SDA:384
    for tt in range(len(AllConCon)):                                                                           # SDA:387-391
        summe = sum([AllConCon[tt][ttt] for ttt in range(len(AllConCon[tt]))])
        for ttt in range(len(AllConCon[tt])):
            if summe > 0.0:
                AllConCon[tt][ttt] /= summe
    return AllConCon


def best_columns(AllConCon):
    """The scan of SDA:399-405 over every column (the script scans as many columns as there are rows: its matrices are
    square), -1 instead of the script's 0 for a zero row; and whether that value is the largest of its column (ours)."""
    best, conf, mutual = [], [], []
    for t in range(len(AllConCon)):
        maxi = 0.0
        maxtt = -1
        for tt in range(len(AllConCon[t])):
            if AllConCon[t][tt] > maxi:
                maxi = AllConCon[t][tt]
                maxtt = tt
        best.append(maxtt)
        conf.append(maxi)
        mutual.append(maxtt >= 0 and maxi == max(AllConCon[:, maxtt]))
    return np.array(best), np.array(conf), np.array(mutual, dtype=bool)


def decided(AllConCon, eps=1e-9):
    """the condition of the exact comparison of best / mutual: in every non-zero row the largest and the second largest value
    differ by more than eps, and so do those of every column that is some row's best"""
    M = np.asarray(AllConCon)
    best = best_columns(M)[0]
    lines = [M[t] for t in range(len(M)) if M[t].max() > 0] + [M[:, b] for b in set(best.tolist()) if b >= 0]
    for v in lines:
        s = np.sort(v)[::-1]
        if len(s) > 1 and s[0] - s[1] <= eps:
            return False
    return True
