// restates the data split of AlphaZeroNN::trainCrossValidation (alphazero_nn.cpp:412-460) for fold 0 and the shuffles of its first
// epoch with libstdc++'s std::shuffle on minstd_rand0 seeded with a raw state: record indices of the training set (in the order its
// minibatches are taken), of the validation set, then the engine state; reference for tests/test_host_cli_analysis.py
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <random>
#include <vector>
int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int n = atoi(argv[1]), k = atoi(argv[2]);
    std::minstd_rand0 eng((unsigned)strtoul(argv[3], nullptr, 10));
    std::vector<int> all(n);
    std::iota(all.begin(), all.end(), 0);
    std::shuffle(all.begin(), all.end(), eng);   // vi % k == 0
    const int start = 0, end = n / k;            // vi = 0
    std::vector<int> tr, va;
    for (int i = 0; i < n; i++) (start < i && i < end ? va : tr).push_back(all[i]);
    std::shuffle(tr.begin(), tr.end(), eng);     // epoch 0
    std::shuffle(va.begin(), va.end(), eng);
    for (int x : tr) printf("%d ", x);
    printf("\n");
    for (int x : va) printf("%d ", x);
    printf("\n");
    std::cout << eng << "\n";
    return 0;
}
